"""CPU reference of the configurable criterion (weights, label smoothing, ignore label, sum / mean, focal term) in torch,
in the dtype of the logits it is given (the tests hand it float64 casts of the SAME f32 logits the kernels read), and
oracle.cova_oracle.loss_and_grads repeated with that criterion in place of CrossEntropyLoss(reduction="sum")."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import cova_oracle as O


def criterion(logits, labels, weight=None, label_smoothing=0.0, focal_gamma=0.0, ignore_index=None, reduction="sum"):
    """Scalar loss (differentiable with respect to ``logits``).  Cross-entropy is F.cross_entropy itself; the focal loss
    is w[y] (1-p_y)^g (-log p_y) over the kept rows, divided by the sum of their w[y] for "mean"."""
    w = None if weight is None else torch.as_tensor(weight).to(logits.dtype)
    if focal_gamma == 0.0:
        return F.cross_entropy(logits, labels, weight=w, ignore_index=-100 if ignore_index is None else ignore_index,
                               label_smoothing=label_smoothing, reduction=reduction)
    assert label_smoothing == 0.0
    keep = torch.ones_like(labels, dtype=torch.bool) if ignore_index is None else labels != ignore_index
    lg, lb = logits[keep], labels[keep]
    logp = F.log_softmax(lg, dim=1).gather(1, lb.view(-1, 1)).view(-1)
    wy = torch.ones_like(logp) if w is None else w[lb]
    num = (wy * (1.0 - logp.exp()) ** focal_gamma * (-logp)).sum()
    return num / wy.sum() if reduction == "mean" else num


def loss_and_dlogits(logits_f32, labels, **kw):
    """float64 loss and dlogits of ``criterion`` on f32 logits cast up (input rounding is not counted as error)."""
    lg = logits_f32.detach().cpu().double().requires_grad_(True)
    loss = criterion(lg, labels.cpu(), **kw)
    loss.backward()
    return loss.detach(), lg.grad


def loss_and_grads(sd, batch, cfg, training=True, **kw):
    """O.loss_and_grads with the criterion swapped -> (loss, logits, grads, sd_after)."""
    work = O.clone_state_dict(sd)
    leaves = {}
    for k in O.param_keys(work):
        work[k] = work[k].clone().requires_grad_(True)
        leaves[k] = work[k]
    logits, _ = O.forward(work, batch["images"], batch["bboxes"], batch["additional_feats"], batch["context_indices"],
                          cfg, training, None, return_intermediates=True)
    loss = criterion(logits, batch["labels"], **kw)
    loss.backward()
    grads = OrderedDict((k, (v.grad if v.grad is not None else torch.zeros_like(v)).detach().clone())
                        for k, v in leaves.items())
    after = OrderedDict((k, v.detach().clone()) for k, v in work.items())
    return loss.detach(), logits.detach(), grads, after
