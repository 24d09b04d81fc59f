"""What the trainer suites share: a small resident page split, seeded weights, the tiny trainer's weights and batches, five
reproducible steps and a parameter count.  Host-side construction only; nothing here needs a device at import time."""
import functools

import numpy as np
import torch

from cova_web_object_detection_amd import synthetic, weights
from config_cases import TRAINER_CFG, spec_of
from helpers import DEV


def page_set(P=15, img=96, seed=4):
    """P pages of img x img uint8 pixels with 11..39 boxes each (x, y, w, h, label), classes 1, 2, 3 once a page"""
    rs = np.random.RandomState(seed)
    u8 = rs.randint(0, 256, (P, img, img, 3)).astype(np.uint8)
    rows = []
    for _ in range(P):
        n = int(rs.randint(11, 40))
        wh = rs.uniform(6, 40, (n, 2))
        xy = rs.uniform(0, 1, (n, 2)) * (img - wh)
        lab = np.zeros((n, 1))
        lab[rs.permutation(n)[:3], 0] = [1, 2, 3]
        rows.append(np.concatenate([xy, wh, lab], 1).astype(np.float32))
    return u8, rows


def seeded(cfg, seed=77, gain=2.0):
    return weights.seeded_state_dict(seed, logit_gain=gain, **spec_of(cfg))


def n_params(cfg):
    spec = weights.state_dict_spec(**spec_of(cfg))
    return sum(int(np.prod(s)) for k, s in spec if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))


def five_steps(tr, ds):
    losses = [tr.train_step(batch)[0] for batch in ds.batches(3, shuffle=True, sampling_fraction=0.9, seed=12, epoch=0)]
    assert len(losses) == 5 and all(np.isfinite(float(x)) for x in losses)
    return [float(x) for x in losses], tr.state_dict()


def trainer_setup(seed=77):
    """TRAINER_CFG's seeded weights and three host batches of two 96-pixel pages"""
    batches = [synthetic.make_batch(2, img_h=96, boxes_per_page=[20 + 3 * i, 11 + 2 * i], context_size=6, seed=900 + i)
               for i in range(3)]
    return seeded(TRAINER_CFG, seed), batches


def no_decay(k):
    """the keys AdamW's decay leaves out in the trainer suites: biases and BatchNorm parameters"""
    return k.endswith(".bias") or ".bn" in k


def dev_batch(b):
    return {k: v.to(DEV) for k, v in b.items() if torch.is_tensor(v)}


@functools.lru_cache(maxsize=None)
def device_setup(seed=77):
    """trainer_setup with the batches on the device, built once"""
    sd, batches = trainer_setup(seed)
    return sd, [dev_batch(b) for b in batches]
