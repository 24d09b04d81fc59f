#!/usr/bin/env python3
"""Generate tests/golden/collate_sampled.npz by running the REFERENCE's WebDataset / custom_collate_fn with
sampling_fraction < 1 (dev container only; see generate_fixtures.py, whose case_collate_raw this follows).

    python tests/golden/generate_sampling_fixture.py        # needs /root/reference (read-only)

The fixture holds the raw inputs (uint8 HWC pixels, the x,y,w,h,label rows and the additional-feature rows as np.loadtxt
returns them), every permutation the reference drew from the seeded np.random, and the reference's outputs per fraction.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "_standin"))
sys.path.insert(0, REF)

import torchvision  # noqa: E402,F401  (the stand-in)
import datasets as ref_datasets  # noqa: E402

assert ref_datasets.__file__.startswith(REF), ref_datasets.__file__

FRACTIONS = (0.9, 0.5)


def case_collate_sampled():
    from PIL import Image
    rs = np.random.RandomState(31)
    counts, cs, H, W, A = [11, 40, 2, 23, 90, 7], 4, 20, 28, 3
    with tempfile.TemporaryDirectory() as d:
        for sub in ("imgs", "bboxes", "additional_features"):
            os.makedirs("%s/%s" % (d, sub))
        ids, u8, rows, addl = [], [], [], []
        for p, n in enumerate(counts):
            img = (rs.uniform(0, 256, (H, W, 3))).astype(np.uint8)
            Image.fromarray(img).save("%s/imgs/%d.png" % (d, p))
            u8.append(img)
            xywh = rs.uniform(1, 12, (n, 4)).astype(np.float32)
            lab = np.zeros((n, 1), dtype=np.float32)
            k = min(3, n)
            lab[rs.permutation(n)[:k], 0] = [1, 2, 3][:k]                  # labelled boxes at random positions
            np.savetxt("%s/bboxes/%d.csv" % (d, p), np.concatenate([xywh, lab], 1), delimiter=",",
                       header="x,y,w,h,label", comments="", fmt="%.6f")
            np.savetxt("%s/additional_features/%d.csv" % (d, p), rs.standard_normal((n, A)), delimiter=",",
                       header=",".join("f%d" % a for a in range(A)), comments="", fmt="%.6f")
            rows.append(np.loadtxt("%s/bboxes/%d.csv" % (d, p), delimiter=",", skiprows=1,
                                   dtype="float32").reshape(n, 5))          # datasets.py:52-60
            addl.append(np.loadtxt("%s/additional_features/%d.csv" % (d, p), delimiter=",", skiprows=1,
                                   dtype="float32").reshape(n, A))          # datasets.py:64-72
            ids.append(str(p))
        out = dict(counts=np.asarray(counts), context_size=cs, u8_pages=np.stack(u8), rows=np.concatenate(rows, 0),
                   additional_feats_in=np.concatenate(addl, 0), fractions=np.asarray(FRACTIONS))
        drawn = []
        real_permutation = np.random.permutation

        def recording_permutation(n):
            perm = real_permutation(n)
            drawn.append(np.asarray(perm).copy())
            return perm

        for f, sf in enumerate(FRACTIONS):
            ds = ref_datasets.WebDataset(d, ids, cs, True, sf)
            np.random.seed(1000 + f)
            del drawn[:]
            np.random.permutation = recording_permutation
            try:
                items = [ds[i] for i in range(len(ids))]
            finally:
                np.random.permutation = real_permutation
            assert [len(p) for p in drawn] == counts
            img_ids, images, bboxes, af, ctx, labels = ref_datasets.custom_collate_fn(items)
            tag = "sf%d/" % f
            out[tag + "perms"] = np.concatenate(drawn)
            out[tag + "bboxes"], out[tag + "labels"] = bboxes.numpy(), labels.numpy()
            out[tag + "context_indices"], out[tag + "additional_feats"] = ctx.numpy(), af.numpy()
            out[tag + "kept_per_page"] = np.asarray([it[2].shape[0] for it in items])
            if f == 0:
                out["images"] = images.numpy()
            print("collate_sampled sf=%g ok" % sf, tuple(bboxes.shape), tuple(ctx.shape), tuple(af.shape))
    np.savez_compressed(os.path.join(HERE, "collate_sampled.npz"), **out)


if __name__ == "__main__":
    case_collate_sampled()
