"""Stage functions of the hot path: each composes C-ABI calls (libcova_hip.so) on device
buffers owned by PyTorch.  No arithmetic of the path is done by torch operators here --
torch only allocates HBM and provides the stream.

Stages: conv stack R1, RoIPool R2, positional encoder R3, optional
additional-feature BN R4, GAT G1-G6, decoder D, loss/predictions L/P, optimizer U.
``params`` maps the reference's state_dict keys (weights.state_dict_spec) to device tensors.
"""
import ctypes
import os

import torch

from . import _lib
from .weights import BACKBONE_CHANNELS as C64, CONTEXT_LAYERS, head_layout

# COVA_GAT_MAX_K of include/cova_hip.h (tests/test_host_cpu.py holds the two equal): neighbour slots per node, up to sixteen
# 64-lane passes of a wavefront
GAT_MAX_K = 1024

call, query = _lib.call, _lib.query
BN_MOMENTUM, BN_EPS, LEAKY_SLOPE = 0.1, 1e-5, 0.2   # nn.BatchNorm defaults; models.py:156


# ------------------------------------------------------------------------------- per-layer modes, gradient plan
# ``training`` of the forward stages is a bool (every layer in that mode: model.train() / model.eval()) or a mapping
# {BatchNorm prefix ("convnet.1.", "convnet.4.0.bn1.", "decoder.2.", ...) or Dropout name ("decoder.0", "decoder.3"): bool}
# (per-module .training, e.g. ``model.train(); model.convnet.eval()``); layers the mapping does not name are in train mode.
# An eval-mode BatchNorm normalises with its running statistics and leaves its buffers alone; an eval-mode Dropout is the
# identity.  A model built with ``attention_dropout`` > 0 also names the Dropout of every attention head, "<head prefix>attn_drop"
# ("gat.attn_drop", "gat.layers.0.heads.1.attn_drop": ATTN_DROP_KEY behind weights.gat_prefixes).
# A model built with ``page_attention_dropout`` / ``page_encoder_dropout`` > 0 names the one Dropout of that layer:
# PAGE_ATTN_DROP_KEY / PAGE_ENC_DROP_KEY.
DROPOUT_KEYS = ("decoder.0", "decoder.3")
ATTN_DROP_KEY = "attn_drop"
PAGE_ATTN_DROP_KEY = "page_attention.attn_drop"
PAGE_ENC_DROP_KEY = "page_encoder.drop"


def is_train(training, key):
    """train (True) / eval (False) flag of the layer ``key`` under ``training`` (a bool or a per-layer mapping)."""
    if isinstance(training, bool):
        return training
    if hasattr(training, "get"):
        return bool(training.get(key, True))
    return bool(training)


def collapse_modes(modes):
    """{layer: bool} -> the bool when every layer shares one mode (then the launches are exactly those of the bool)."""
    vals = set(bool(v) for v in modes.values())
    return vals.pop() if len(vals) == 1 else dict(modes)


# Backward stages that a gradient plan may leave out (grad_plan):
#   "convstack"   RoIPool / RoIAlign backward + the whole conv-stack backward (the forward then keeps no activations)
#   "stem"        block 0's first data gradient (its residual into the pool output included), the stem BatchNorm / ReLU /
#                 max-pool backward (resnet50: the first Bottleneck's input gradient)
#   "conv1_wgrad" the 7x7 conv1 weight gradient (cova_conv1_wgrad*)
#   "wgrad:K"     the weight gradient of layer1 convolution K (a state_dict key; the 3x3 ones and the resnet50 conv1 1x1s)
#   "bbox"        the positional encoder's backward; "addl" the additional-feature BatchNorm's backward
# with the optional layer2 stage (``layer2=True``, backbone_layers=2) also:
#   "layer1"      layer2 block 0's data gradients into layer1's output (3x3 s2 and 1x1 s2, one launch) and everything of
#                 layer1 and below; "wgrad:convnet.5.K" the weight gradient of layer2 convolution K
PLAN_STAGES = ("convstack", "stem", "conv1_wgrad", "bbox", "addl", "layer1")


def grad_plan(need, want_dimg=False, layer2=False):
    """(state_dict keys of the parameters that need a gradient, images need one?) -> frozenset of the backward stages to
    issue.  A stage is left out only when nothing downstream of it is wanted; every other pattern computes more than it
    needs (the caller drops the gradients of frozen parameters).  ``layer2``: the model has the layer2 stage."""
    need = set(need)
    plan = set()
    if any(k.startswith("bbox_feat_encoder.") for k in need):
        plan.add("bbox")
    if any(k.startswith("bn_additional_feat.") for k in need):
        plan.add("addl")
    if want_dimg or any(k.startswith("convnet.") for k in need):
        plan.add("convstack")
        if want_dimg or need & {"convnet.0.weight", "convnet.1.weight", "convnet.1.bias"}:
            plan.add("stem")
        if "convnet.0.weight" in need:
            plan.add("conv1_wgrad")
        plan.update("wgrad:" + k for k in need if k.startswith("convnet.4.") and ".conv" in k)
        if layer2:
            if want_dimg or any(k.startswith(("convnet.0.", "convnet.1.", "convnet.4.")) for k in need):
                plan.add("layer1")
            plan.update("wgrad:" + k for k in need if k.startswith("convnet.5.") and k.endswith(("conv1.weight",
                                                                                              "conv2.weight",
                                                                                              "downsample.0.weight")))
    return frozenset(plan)


def has_layer2(params):
    return "convnet.5.0.conv1.weight" in params


def full_plan(params):
    """The plan of a step in which every parameter of ``params`` needs its gradient (no stage left out)."""
    return grad_plan(list(params), layer2=has_layer2(params))


def on_device_of(argpos):
    """Run an engine entry point under the device guard of its tensors (argument `argpos`): the host-side size
    queries (persistent-grid sizes, workspace sizes) then consult the SAME device the launches go to -- the reference
    picks `cuda:<-d>` without ever calling set_device (main.py:17), so the process' current device may be another GPU."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapped(*args, **kw):
            t = args[argpos]
            t = t.get("images") if isinstance(t, dict) else t
            if isinstance(t, torch.Tensor) and t.is_cuda and t.device.index != torch.cuda.current_device():
                with torch.cuda.device(t.device):
                    return fn(*args, **kw)
            return fn(*args, **kw)
        return wrapped
    return deco


def _empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def _gbuf(gout, key, shape, like):
    """Gradient destination: the caller's view (flat all-reduce bucket) or a fresh tensor."""
    if gout is not None and key in gout:
        g = gout[key]
        assert g.numel() == int(torch.Size(shape).numel()) and g.is_contiguous(), key
        return g
    return _empty(shape, like)


def _check(t, dtype=torch.float32):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return t


def check_batch(cfg, images, bboxes, additional_feats, context_indices, training, visual_feats=None):
    """Shape contract of CoVA.forward (models.py:94-122), checked on the host before any launch (the
    kernels take raw pointers): the errors torch raises inside the reference's forward for malformed
    input -- conv2d's channel check, the [N,5] roi layout, the cat/Linear width mismatch, gather
    broadcasting, BatchNorm1d's train-mode batch-size check -- with the same exception types.
    Index VALUES are not read here (that would cost a device sync): ids outside [0, N) are treated
    as pads by the kernels, memory-safe; the reference raises IndexError for them on CPU.
    With ``visual_feats`` (cached RoI features, check_visual_feats) ``images`` may be None."""
    if images is None:
        if visual_feats is None:
            raise RuntimeError("a batch without images needs cached visual features (visual_feats)")
    elif images.dim() != 4 or images.shape[1] != 3:
        raise RuntimeError("expected images [B, 3, H, W] (conv1 has 3 input channels, models.py:49), got %s"
                           % (tuple(images.shape),))
    if bboxes.dim() != 2 or bboxes.shape[1] != 5:
        raise RuntimeError("expected bboxes [N, 5] = [batch_idx, x1, y1, x2, y2] (models.py:97), got %s"
                           % (tuple(bboxes.shape),))
    N, A = bboxes.shape[0], cfg["n_additional_feat"]
    if visual_feats is not None:
        check_visual_feats(cfg, visual_feats, N)
    if additional_feats.dim() != 2 or tuple(additional_feats.shape) != (N, A):
        raise RuntimeError("expected additional_feats [%d, %d] (n_additional_feat, models.py:98,110), got %s"
                           % (N, A, tuple(additional_feats.shape)))
    if cfg["use_context"]:
        if context_indices.dim() != 2 or context_indices.shape[0] != N:
            raise RuntimeError("expected context_indices [%d, 2*context_size] (models.py:99), got %s"
                               % (N, tuple(context_indices.shape)))
        if context_indices.is_floating_point() or context_indices.dtype == torch.bool:
            raise IndexError("context_indices must be an integer tensor (models.py:186 indexes with it)")
        if context_indices.shape[1] > GAT_MAX_K:
            raise ValueError("n_context > %d (-cs > %d) is not supported by the wave-per-node kernel"
                             % (GAT_MAX_K, GAT_MAX_K // 2))
    if N == 1:
        # torch.nn.functional.batch_norm's _verify_batch_size, hit by the first train-mode BatchNorm1d of the forward
        for width, prefix in ((cfg["bbox_hidden_dim"], "bbox_feat_encoder.1."), (A, "bn_additional_feat."),
                              (head_layout(cfg, backbone_feat(cfg)).T, "decoder.2.")):
            if width and is_train(training, prefix):
                raise ValueError("Expected more than 1 value per channel when training, got input size "
                                 "torch.Size([1, %d])" % width)


def backbone_feat(cfg):
    PH, PW = cfg["roi_output_size"]
    from .weights import backbone_channels
    return backbone_channels(cfg.get("backbone", "resnet18"), cfg.get("backbone_layers", 1)) * PH * PW


def feature_map_size(n, backbone_layers=1):
    """conv1 (7,2,3) then maxpool (3,2,1): models.py:53-56 does this with a dummy forward; layer2's first conv (3,2,1)
    halves it once more."""
    n = query("cova_conv_out_size", query("cova_conv_out_size", n, 7, 2, 3), 3, 2, 1)
    return query("cova_conv_out_size", n, 3, 2, 1) if backbone_layers == 2 else n


# ------------------------------------------------------------------------------- BatchNorm
class BNState:
    """scale/shift/mean/invstd of one BatchNorm application (+ what backward needs)."""
    __slots__ = ("scale", "shift", "mean", "invstd", "count", "C", "abc", "frozen")


FOLD_ABOVE, FOLD_GROUP = 256, 64


def fold_partials(partial, nparts, width):
    """Pre-reduce a long list of partial rows so the single-block finalize kernels stay short."""
    while nparts > FOLD_ABOVE:
        n2 = (nparts + FOLD_GROUP - 1) // FOLD_GROUP
        out = _empty((n2, width), partial)
        call("cova_partials_fold", partial, nparts, width, FOLD_GROUP, out)
        partial, nparts = out, n2
    return partial, nparts


# Optional SyncBN (SURVEY.md section 8e "exact large-batch mode"): while STAT_SYNC is set (by the
# trainer, for the duration of one training step) every BatchNorm statistic row -- (sum x, sum x^2)
# forward, (sum dy, sum dy*xhat) backward -- is summed over the data-parallel group before it is
# finalized, with the element count scaled to the whole batch.  Messages are 2*C floats.
class StatSync:
    def __init__(self, group, ratio_pages, ratio_boxes):
        self.group = group
        self.ratio = {"pages": float(ratio_pages), "boxes": float(ratio_boxes)}   # global / local count

    def all_reduce(self, row):
        import torch.distributed as dist
        dist.all_reduce(row, op=dist.ReduceOp.SUM, group=self.group)


STAT_SYNC = None


def _global_stats(partial, nparts, width, count, unit):
    """Local partial rows -> ONE row summed over all ranks, and the count of the whole batch."""
    row = _empty((1, width), partial)
    call("cova_partials_fold", partial, nparts, width, max(int(nparts), 1), row)
    STAT_SYNC.all_reduce(row)
    return row, 1, count * STAT_SYNC.ratio[unit]


def bn_finalize_bwd(part, nparts, C, count, dgamma, dbeta, unit, abc_from=None, frozen=False):
    """cova_bn_finalize_bwd (-> coef [2,C]) or, with ``abc_from`` = the layer's BNState,
    cova_bn_finalize_bwd_abc (-> A|B|C [3,C]).  Under SyncBN the parameter gradients come from the
    LOCAL sums (the gradient exchange adds the ranks up) and the dz coefficients from the sums and
    the count of the whole batch (torch.nn.SyncBatchNorm's backward does the same).
    ``frozen`` (eval-mode BatchNorm, running statistics): the layer is a fixed per-channel affine, so
    dz = scale*dy -- the batch-coupling terms are dropped (A = scale, B = C = 0 / coef = 0) while
    dgamma = sum dy*xhat and dbeta = sum dy keep their meaning (torch's eval-mode batch_norm backward)."""
    part, nparts = fold_partials(part, nparts, 2 * C)
    out = _empty((3 if abc_from is not None else 2, C), part)

    def fin(p, n, cnt, dg, db):
        if abc_from is not None:
            call("cova_bn_finalize_bwd_abc", p, n, C, float(cnt), dg, db, abc_from.mean, abc_from.invstd,
                 abc_from.scale, out)
        else:
            call("cova_bn_finalize_bwd", p, n, C, float(cnt), dg, db, out)

    fin(part, nparts, count, dgamma, dbeta)
    if STAT_SYNC is not None and not frozen:            # (an eval-mode layer has no batch coupling to exchange)
        gp, gn, gc = _global_stats(part, nparts, 2 * C, count, unit)
        scratch = _empty((2, C), part)
        fin(gp, gn, gc, scratch[0], scratch[1])
    if frozen:
        out.zero_()
        if abc_from is not None:
            out[0].copy_(abc_from.scale)
    return out


def bn_state(C, like, count, training):
    st = BNState()
    st.C, st.count, st.frozen = C, float(count), not training
    st.abc = _empty((3, C), like)               # scale | (unused) | shift: the prologue's A | B | C
    st.scale, st.shift = st.abc[0], st.abc[2]
    st.mean, st.invstd = _empty((C,), like), _empty((C,), like)
    return st


def tails_on(C=C64):
    """in-launch BatchNorm finalize: 64-channel producers, no SyncBN (a collective sits between partials and finalize)"""
    return OPTIONS.bn_tail and STAT_SYNC is None and C == C64


def bn_tail_fwd(prefix, params, buffers, C, like, count, update_running=True):
    """(BNState, BnTail) for a train-mode BatchNorm whose statistics the NEXT launch produces: the tail writes
    scale / shift / mean / invstd and the running statistics, as cova_bn_finalize_fwd would."""
    st = bn_state(C, like, count, True)
    upd = update_running
    tail = BnTail(1, like, count, gamma=params[prefix + "weight"], beta=params[prefix + "bias"],
                  running_mean=buffers[prefix + "running_mean"] if upd else None,
                  running_var=buffers[prefix + "running_var"] if upd else None,
                  num_batches_tracked=buffers.get(prefix + "num_batches_tracked") if upd else None,
                  scale=st.scale, shift=st.shift, mean=st.mean, invstd=st.invstd)
    return st, tail


def bn_tail_bwd(st, count, gout, prefix, like):
    """(dgamma, dbeta, abc, BnTail): the launch that produces the (sum g, sum g*xhat) partials of BatchNorm `st` also
    writes its parameter gradients and the dz = abc[0]*dy + abc[1]*z + abc[2] coefficients."""
    C = st.C
    dgamma = _gbuf(gout, prefix + "weight", (C,), like)
    dbeta = _gbuf(gout, prefix + "bias", (C,), like)
    abc = _empty((3, C), like)
    tail = BnTail(2, like, count, mean=st.mean, invstd=st.invstd, scale=st.scale, dgamma=dgamma, dbeta=dbeta, abc=abc)
    return dgamma, dbeta, abc, tail


def bn_params(prefix, params, buffers, C, like, training, partial=None, nparts=0, count=0,
              update_running=True, unit="boxes"):
    training = is_train(training, prefix)
    st = bn_state(C, like, count, training)
    g, b = params[prefix + "weight"], params[prefix + "bias"]
    rm, rv = buffers[prefix + "running_mean"], buffers[prefix + "running_var"]
    if training:
        upd = update_running
        partial, nparts = fold_partials(partial, nparts, 2 * C)
        if STAT_SYNC is not None:
            partial, nparts, count = _global_stats(partial, nparts, 2 * C, count, unit)
            st.count = float(count)
        nbt = buffers.get(prefix + "num_batches_tracked") if upd else None
        call("cova_bn_finalize_fwd", partial, nparts, C, float(count), g, b, rm if upd else None,
             rv if upd else None, nbt, BN_MOMENTUM, BN_EPS, st.scale, st.shift, st.mean, st.invstd)
    else:
        call("cova_bn_eval_params", g, b, rm, rv, BN_EPS, C, st.scale, st.shift, st.mean, st.invstd)
    return st


def colstats(x, ld, R, C):
    n = query("cova_colreduce_num_chunks", R, C)
    part = _empty((n, 2, C), x)
    call("cova_colstats", x, ld, R, C, part)
    return part, n


def bn_backward(dout, ldd, act, lda, z, ldz, st, R, dz, lddz, dres=None, lddres=0, gout=None,
                prefix=None, unit="boxes", drop=None, colsum=None):
    """Returns (dgamma, dbeta); writes dz (and dres = relu-masked dout).  ``drop`` = (mask, p): dout is the gradient
    BEHIND a Dropout of the layer's output (its backward is applied first); ``colsum`` [C]: receives the column sums
    of dz."""
    C = st.C
    if (bn1d_fused(not st.frozen) and dres is None and R > 0 and z.dim() == 2 and dz.data_ptr() != dout.data_ptr()):
        dgamma = _gbuf(gout, (prefix or "") + "weight", (C,), z)
        dbeta = _gbuf(gout, (prefix or "") + "bias", (C,), z)
        call("cova_bn1d_bwd", dout, ldd, drop[0] if drop else None, float(drop[1]) if drop else 0.0, act, lda, z, ldz,
             st.mean, st.invstd, st.scale, R, C, dgamma, dbeta, dz, lddz, colsum)
        return dgamma, dbeta
    if drop is not None:
        dy = _empty((R, C), dout)
        call("cova_dropout_bwd", dout, ldd, drop[0], dy, C, R, C, float(drop[1]))
        dout, ldd = dy, C
    n = query("cova_colreduce_num_chunks", R, C)
    part = _empty((n, 2, C), z)
    call("cova_bn_bwd_reduce", dout, ldd, act, lda, z, ldz, st.mean, st.invstd, R, C, part)
    dgamma = _gbuf(gout, (prefix or "") + "weight", (C,), z)
    dbeta = _gbuf(gout, (prefix or "") + "bias", (C,), z)
    coef = bn_finalize_bwd(part, n, C, R, dgamma, dbeta, unit, frozen=st.frozen)
    call("cova_bn_bwd_apply", dout, ldd, act, lda, z, ldz, st.mean, st.invstd, st.scale, coef, dz,
         lddz, dres, lddres, R, C)
    if colsum is not None:
        call("cova_colsum", dz, lddz, R, C, colsum)
    return dgamma, dbeta


# ------------------------------------------------------------------------------- conv stack
# 3x3 convolutions: Winograd F(4x4,3x3) kernels only (csrc/conv_wino4.hip forward / data gradient, csrc/conv_wgrad4.hip weight
# gradient; the F(2x2,3x3) kernels of rounds 1-3 are a test-support library now, tools/csrc).  BatchNorm+ReLU between
# the two convs of a block and the BatchNorm-backward "apply" passes are evaluated on load inside the consuming
# convolutions: a1 and dz are never written to HBM.
class _BnTailStruct(ctypes.Structure):
    """cova_bn_tail as include/cova_hip.h defines it (a HOST struct of device pointers, read by the launch call)"""
    _fields_ = _lib.parse_struct("cova_bn_tail")


class BnTail:
    """BatchNorm finalize riding on the launch that produces the statistics partials (csrc/bn_tail.h): the struct
    plus the tensors it points to (kept alive until the launch call has returned)."""
    _COUNTERS = {}

    def __init__(self, mode, like, count, **ptrs):
        key = (like.device, torch.cuda.current_stream(like.device).cuda_stream)
        ctr = BnTail._COUNTERS.get(key)
        if ctr is None:                      # one ticket counter per (device, stream): launches on a stream are ordered,
            ctr = BnTail._COUNTERS[key] = torch.zeros((1,), dtype=torch.int32, device=like.device)   # the kernel leaves it 0
        self.keep = [ctr] + [v for v in ptrs.values() if isinstance(v, torch.Tensor)]
        c = _BnTailStruct()
        c.mode, c.counter, c.count = mode, ctr.data_ptr(), float(count)
        c.momentum, c.eps = BN_MOMENTUM, BN_EPS
        for k, v in ptrs.items():
            setattr(c, k, v.data_ptr() if isinstance(v, torch.Tensor) else None)
        self.c = c

    @property
    def ptr(self):
        return ctypes.addressof(self.c)


class Options:
    """The run-time switches of the path (process-wide; read at call time)."""
    # data-parallel steps: the head's gradient all-reduce is issued under the conv-stack backward (trainer.py)
    overlap_allreduce = os.environ.get("COVA_OVERLAP_ALLREDUCE", "1") != "0"
    # BatchNorm finalize as the tail of the producing convolution launch (no separate finalize launches)
    bn_tail = os.environ.get("COVA_BN_TAIL", "1") != "0"


OPTIONS = Options()

CONV3_KEYS = ["convnet.4.0.conv1", "convnet.4.0.conv2", "convnet.4.1.conv1", "convnet.4.1.conv2"]
BN3_KEYS = ["convnet.4.0.bn1.", "convnet.4.0.bn2.", "convnet.4.1.bn1.", "convnet.4.1.bn2."]


class LazyFeature:
    """The last BasicBlock's output relu(bn2(z2) + x) left un-materialised: RoIPool (forward and
    backward mask) forms it on the fly (cova_roipool_fwd_bn / cova_roipool_bwd_bn)."""
    __slots__ = ("z", "x", "scale", "shift", "shape")

    def __init__(self, z, x, scale, shift):
        self.z, self.x, self.scale, self.shift, self.shape = z, x, scale, shift, tuple(z.shape)


def is_bottleneck(params):
    """ResNet-50-stem extension (layer1 = 3 Bottlenecks, 256 channels) vs the reference's ResNet-18."""
    return "convnet.4.0.conv3.weight" in params


@on_device_of(0)
def convstack_fwd(images, params, buffers, training, save=True, lazy_out=False):
    """images NCHW [B,3,H,W] -> feature map NHWC [B,Hf,Wf,C]  (models.py:49-51,125);
    with ``lazy_out`` (Winograd path) a LazyFeature instead of the tensor.  ``training``: a bool or per-BatchNorm modes
    (is_train); ``save``: keep what the backward needs."""
    _check(images)
    B, _, H, W = images.shape
    H1, W1 = query("cova_conv_out_size", H, 7, 2, 3), query("cova_conv_out_size", W, 7, 2, 3)
    H2, W2 = query("cova_conv_out_size", H1, 3, 2, 1), query("cova_conv_out_size", W1, 3, 2, 1)
    bottleneck = is_bottleneck(params)
    layer2 = has_layer2(params)
    lazy_out = lazy_out and not layer2              # layer2 reads layer1's output: materialised
    sv = {"images": images, "dims": (B, H, W, H1, W1, H2, W2), "kind": "bottleneck" if bottleneck else "basic"}
    # the Winograd images of the 3x3 weights: one small launch
    if bottleneck:
        sv["_w3"] = conv3_weights([params["convnet.4.%d.conv2.weight" % b] for b in (0, 1, 2)], images)
    else:
        sv["_w3"] = conv3_weights([params[k + ".weight"] for k in CONV3_KEYS], images)
    # conv1 + bn1 + relu + maxpool
    y1 = _empty((B, H1, W1, C64), images)
    nt1 = query("cova_conv1_num_partials", B, H, W)
    stem_train = is_train(training, "convnet.1.")
    part = _empty((nt1, 2, C64), images) if stem_train else None
    # (the kernel reads the OIHW weight itself: no layout-prep launch)
    if stem_train and tails_on():
        bn1, tail = bn_tail_fwd("convnet.1.", params, buffers, C64, images, B * H1 * W1)
        call("cova_conv1_fwd_tail", images, params["convnet.0.weight"], y1, part, B, H, W, tail.ptr)
    else:
        call("cova_conv1_fwd_tail", images, params["convnet.0.weight"], y1, part, B, H, W, None)
        bn1 = bn_params("convnet.1.", params, buffers, C64, images, training, part, nt1, B * H1 * W1, unit="pages")
    p1 = _empty((B, H2, W2, C64), images)
    idx = _empty((B, H2, W2, C64), images, torch.uint8)
    # ymax = y1 at each window's arg-max: lets the last data-gradient conv take bn1's backward sums
    want_ymax = save and (stem_train or bottleneck)
    ymax = _empty((B, H2, W2, C64), images) if want_ymax else None
    call("cova_bn_relu_maxpool_fwd", y1, bn1.scale, bn1.shift, p1, idx, ymax, B, H1, W1)
    sv.update(y1=y1, bn1=bn1, idx=idx, ymax=ymax)
    if bottleneck:
        feat = _layer1_bottleneck_fwd(p1, params, buffers, training, save, lazy_out, sv)
    else:
        feat = _layer1_basic_fwd(p1, params, buffers, training, save, lazy_out, sv)
    if layer2:
        feat = _layer2_fwd(feat, params, buffers, training, save, sv)
    return feat, (sv if save else None)


def conv3_num_partials(B, H, W):
    return query("cova_conv3x3_wino4_num_partials", B, H, W)


def conv3x3_pro(u, inp, in2, abc, relu, addend, act, msc, msh, z, mean, invstd, out, part, B, H, W, tail=None,
                act_bits=None):
    """conv3x3 of f(A*inp + B*in2 + C) (abc / in2 nullable) with the fused epilogue of cova_conv3x3_wino4_full.
    u = the F(4x4,3x3) weight operand (conv3_weights); tail: BnTail; act_bits (with a tail only): the mask source `act`
    as one bit per element (cova_bn_act_fwd_bits)."""
    if tail is not None:
        if act_bits is not None:
            act = None
        call("cova_conv3x3_wino4_full_tail", inp, in2, abc, relu, u, addend, act, act_bits, msc, msh, z, mean, invstd,
             out, part, B, H, W, tail.ptr)
    else:
        call("cova_conv3x3_wino4_full", inp, in2, abc, relu, u, addend, act, msc, msh, z, mean, invstd, out, part,
             B, H, W)


def conv3_weights(ws, like):
    """3x3 weights (a list of up to four OIHW tensors) -> ([forward operands], [data-gradient operands]) of the F(4x4,3x3)
    kernels, all from ONE launch."""
    n = len(ws)
    uf, ud = _empty((n, query("cova_conv3x3_wino4_u_floats")), like), _empty((n, query("cova_conv3x3_wino4_u_floats")), like)
    call("cova_conv3x3_wino4_prep_multi", *(list(ws) + [None] * (4 - n)), uf, ud)
    return [uf[i] for i in range(n)], [ud[i] for i in range(n)]


def conv_bn_fwd(u, inp, abc, relu, out, prefix, params, buffers, training, part, nt, R, B, H, W):
    """3x3 conv (input relu?(abc . inp) on load) followed by a BatchNorm whose statistics it produces -> BNState.
    An eval-mode BatchNorm (``training`` resolved for ``prefix``) takes no statistics: ``part`` is not written."""
    training = is_train(training, prefix)
    if not training:
        part = None
    if training and tails_on():
        st, tail = bn_tail_fwd(prefix, params, buffers, C64, inp, R)
        conv3x3_pro(u, inp, None, abc, relu, None, None, None, None, None, None, None, out, part, B, H, W, tail)
        return st
    conv3x3_pro(u, inp, None, abc, relu, None, None, None, None, None, None, None, out, part, B, H, W)
    return bn_params(prefix, params, buffers, C64, inp, training, part, nt, R, unit="pages")


def conv_bn_pair_fwd(ua, ub, x, z1, z2, pa, pb, params, buffers, training, part, nt, R, B, H, W):
    """z1 = conv_a(x), bn_a;  z2 = conv_b(relu(bn_a(z1))) with a1 formed on load, bn_b  -> (BNState a, BNState b).
    Each BatchNorm follows its own mode (the tailed form only for a train-mode layer)."""
    bna = conv_bn_fwd(ua, x, None, 0, z1, pa, params, buffers, training, part, nt, R, B, H, W)
    bnb = conv_bn_fwd(ub, z1, bna.abc, 1, z2, pb, params, buffers, training, part, nt, R, B, H, W)
    return bna, bnb


def _layer1_basic_fwd(p1, params, buffers, training, save, lazy_out, sv):
    """layer1 of ResNet-18: two BasicBlocks (the reference's backbone, models.py:49-51)"""
    images = p1
    B, H, W, H1, W1, H2, W2 = sv["dims"]
    wf, wd = sv.pop("_w3")                            # (requested in front of the stem, convstack_fwd)
    sv["wd"] = wd
    R = B * H2 * W2
    nt = conv3_num_partials(B, H2, W2)
    x = p1
    blocks = []
    for blk in (0, 1):
        ta, tb = is_train(training, BN3_KEYS[2 * blk]), is_train(training, BN3_KEYS[2 * blk + 1])
        if not save and not ta and not tb:
            # inference: running statistics are known up front, so BatchNorm (+ residual) + ReLU sit in the conv
            # prologues / epilogues -- two launches per BasicBlock, nothing else touches the maps
            bna = bn_params(BN3_KEYS[2 * blk], params, buffers, C64, images, False)
            bnb = bn_params(BN3_KEYS[2 * blk + 1], params, buffers, C64, images, False)
            ua, ub = wf[2 * blk], wf[2 * blk + 1]
            # conv1 plain; conv2 reads relu(bn1(z1)) formed on load and either carries bn2 + identity + ReLU in its epilogue,
            # or (last block, lazy feature map) leaves them to RoIPool
            z1 = _empty((B, H2, W2, C64), images)
            call("cova_conv3x3_wino4", x, ua, z1, None, B, H2, W2)
            if blk == 1 and lazy_out:
                z2 = _empty((B, H2, W2, C64), images)
                call("cova_conv3x3_wino4_pro", z1, bna.abc, 1, ub, z2, None, B, H2, W2)
                feat = LazyFeature(z2, x, bnb.scale, bnb.shift)
                blocks.append(dict(x=x, z1=z1, a1=None, z2=z2, out=None, bna=bna, bnb=bnb))
                continue
            out = _empty((B, H2, W2, C64), images)
            call("cova_conv3x3_wino4_bnact", z1, bna.abc, 1, ub, x, bnb.scale, bnb.shift, 1, out, B, H2, W2)
            blocks.append(dict(x=x, z1=z1, a1=None, z2=None, out=out, bna=bna, bnb=bnb))
            x = feat = out
            continue
        part = _empty((nt, 2, C64), images) if ta or tb else None
        z1, z2 = _empty((B, H2, W2, C64), images), _empty((B, H2, W2, C64), images)
        bna, bnb = conv_bn_pair_fwd(wf[2 * blk], wf[2 * blk + 1], x, z1, z2, BN3_KEYS[2 * blk], BN3_KEYS[2 * blk + 1],
                                    params, buffers, training, part, nt, R, B, H2, W2)
        out_bits = None
        if blk == 1 and lazy_out:
            out = None
            feat = LazyFeature(z2, x, bnb.scale, bnb.shift)
        else:
            out = _empty((B, H2, W2, C64), images)
            if blk == 0 and save and tb and tails_on():
                # ... with its ReLU decisions as bits: the mask source of the next block's conv1 data gradient
                out_bits = _empty((R, 2), images, torch.int32)
                call("cova_bn_act_fwd_bits", z2, bnb.scale, bnb.shift, x, out, out_bits, R)
            else:
                call("cova_bn_act_fwd", z2, C64, bnb.scale, bnb.shift, x, C64, out, C64, R, C64, 1)
            feat = out
        blocks.append(dict(x=x, z1=z1, a1=None, z2=z2, out=out, bna=bna, bnb=bnb, out_bits=out_bits))
        x = out
    sv["blocks"] = blocks
    # what RoIPool's backward needs of the block that produced the feature map
    last = blocks[1]
    sv["last"] = dict(out=last["out"], x=last["x"], z=last["z2"], bn=last["bnb"], prefix=BN3_KEYS[3])
    return feat


# ---- ResNet-50-stem extension: layer1 = 3 torchvision Bottlenecks (conv1x1 Cin->64, bn, relu, conv3x3
# 64->64, bn, relu, conv1x1 64->256, bn, (+ downsample conv1x1 64->256 + bn in block 0), add, relu).
# Same structure as the BasicBlock path: every BatchNorm(+ReLU) between convs is applied on load by the
# consumer, statistics come from the producers' epilogues, the last block's output stays un-materialised.
C256 = 4 * C64


def conv1x1(inp, in2, abc, relu, w, w_trans, out, part, R, cin, cout, addend=None, act=None, msc=None,
            msh=None, z=None, mean=None, invstd=None, z2=None, mean2=None, invstd2=None, part2=None, act_bits=None):
    call("cova_conv1x1", inp, in2, abc, 1 if relu else 0, w, 1 if w_trans else 0, addend, act, act_bits, msc, msh,
         z, mean, invstd, z2, mean2, invstd2, out, part, part2, R, cin, cout)


def _layer1_bottleneck_fwd(p1, params, buffers, training, save, lazy_out, sv):
    B, H, W, H1, W1, H2, W2 = sv["dims"]
    R = B * H2 * W2
    nt = conv3_num_partials(B, H2, W2)

    def stats(cin, cout, prefix):
        n = query("cova_conv1x1_num_partials", R, cin, cout)
        return (_empty((n, 2, cout), p1) if is_train(training, prefix) else None), n

    def bn(prefix, C, part, n):
        return bn_params(prefix, params, buffers, C, p1, training, part, n, R, unit="pages")

    ufs, uds = sv.pop("_w3")
    x, cin, blocks, feat = p1, C64, [], None
    pending = None      # (z3, other, abc): the previous block's output relu(abc . (z3, other)), not yet written
    for blk in (0, 1, 2):
        pre = "convnet.4.%d." % blk
        s = dict(cin=cin, pre=pre)
        part, n = stats(cin, C64, pre + "bn1.")
        s["z1"] = _empty((B, H2, W2, C64), p1)
        if pending is None:
            conv1x1(x, None, None, 0, params[pre + "conv1.weight"], 0, s["z1"], part, R, cin, C64)
        else:
            # the block input is materialised by its first consumer (one pass over the 256-channel map less
            # than a separate bn + residual + ReLU kernel)
            x = _empty((B, H2, W2, C256), p1)
            # ... together with its ReLU decisions, one bit per element: the mask source of this block's input gradient
            s["x_bits"] = (_empty((R, C256 // 32), p1, torch.int32)
                           if save and is_train(training, "convnet.4.%d.bn3." % (blk - 1)) else None)
            call("cova_conv1x1_materialize", pending[0], pending[1], pending[2], params[pre + "conv1.weight"], x,
                 s["x_bits"], s["z1"], part, R)
            blocks[-1]["out"] = x
        s["x"] = x
        s["bn1"] = bn(pre + "bn1.", C64, part, n)
        uf, s["ud"] = ufs[blk], uds[blk]
        part = _empty((nt, 2, C64), p1) if is_train(training, pre + "bn2.") else None
        s["z2"] = _empty((B, H2, W2, C64), p1)
        s["bn2"] = conv_bn_fwd(uf, s["z1"], s["bn1"].abc, 1, s["z2"], pre + "bn2.", params, buffers, training, part, nt,
                               R, B, H2, W2)
        part, n = stats(C64, C256, pre + "bn3.")
        s["z3"] = _empty((B, H2, W2, C256), p1)
        conv1x1(s["z2"], None, s["bn2"].abc, 1, params[pre + "conv3.weight"], 0, s["z3"], part, R, C64, C256)
        s["bn3"] = bn(pre + "bn3.", C256, part, n)
        bn3 = s["bn3"]
        s["out"] = None
        if blk == 0:
            part, n = stats(C64, C256, pre + "downsample.1.")
            s["zd"] = _empty((B, H2, W2, C256), p1)
            conv1x1(x, None, None, 0, params[pre + "downsample.0.weight"], 0, s["zd"], part, R, C64, C256)
            s["bnd"] = bn(pre + "downsample.1.", C256, part, n)
            abc = _empty((3, C256), p1)          # out = relu(s3*z3 + sd*zd + (h3 + hd))
            abc[0].copy_(bn3.scale)
            abc[1].copy_(s["bnd"].scale)
            torch.add(bn3.shift, s["bnd"].shift, out=abc[2])
            pending = (s["z3"], s["zd"], abc)
        elif blk == 1:
            bn3.abc[1].fill_(1.0)                # out = relu(s3*z3 + 1*x + h3): the unused B row of scale | . | shift
            pending = (s["z3"], x, bn3.abc)
        elif lazy_out:
            feat = LazyFeature(s["z3"], x, bn3.scale, bn3.shift)
        else:
            s["out"] = _empty((B, H2, W2, C256), p1)
            call("cova_bn_act_fwd", s["z3"], C256, bn3.scale, bn3.shift, x, C256, s["out"], C256, R, C256, 1)
            feat = s["out"]
        blocks.append(s)
        cin = C256
    sv["blocks"] = blocks
    last = blocks[2]
    sv["last"] = dict(out=last["out"], x=last["x"], z=last["z3"], bn=last["bn3"])
    return feat


def bn_act(z, st, res=None, relu=True):
    """relu?(bn(z) (+ res)) materialised with the same fma the fused prologues evaluate (tests, tools)."""
    C = st.C
    out = torch.empty_like(z)
    call("cova_bn_act_fwd", z, C, st.scale, st.shift, res, C if res is not None else 0, out, C,
         z.numel() // C, C, 1 if relu else 0)
    return out


_IDENT_ABC = {}


def _ident_abc(like):
    """A | B | C = 1 | 0 | 0 for 64 channels (an operand that needs no affine prologue), cached per device."""
    t = _IDENT_ABC.get(like.device)
    if t is None:
        t = torch.zeros((3, C64), device=like.device)
        t[0].fill_(1.0)
        _IDENT_ABC[like.device] = t
    return t


def _lin_conv_bn_bwd(v, act, act_abc, act_relu, w, st, R, gout, bn_prefix, w_key, grads, ws):
    """Backward of (1x1 conv 64->256, BatchNorm ``st``) in linear form (csrc/conv1x1_lin.hip): parameter
    gradients of both, and (avec, m, cvec) = the operands of cova_conv1x1_lin_dgrad.  ``v`` = masked gradient
    w.r.t. the BatchNorm output, ``act`` (+ affine/ReLU on load) = the conv's input.  The conv output is not read."""
    lin = _empty((query("cova_conv1x1_lin_floats"),), v)
    call("cova_conv1x1_vprod", v, act, act_abc, 1 if act_relu else 0, lin, ws, R)
    part = _empty((1, 2, C256), v)
    call("cova_conv1x1_lin_bnsums", lin, w, st.mean, st.invstd, part)
    dg, db, abc = _bn_abc_from_partials(part, 1, st, R, gout, bn_prefix, v)
    grads[bn_prefix + "weight"], grads[bn_prefix + "bias"] = dg, db
    dw = _gbuf(gout, w_key, (C256, C64, 1, 1), v)
    m, cvec, avec = _empty((C64, C64), v), _empty((C64,), v), _empty((3, C256), v)
    call("cova_conv1x1_lin_finish", lin, abc, w, dw, m, cvec, avec)
    grads[w_key] = dw
    return avec, m, cvec


def _layer1_bottleneck_bwd(sv, g, params, gout, grads, head_part, plan=None):
    """Backward of the three Bottlenecks.  ``g`` = gradient w.r.t. the last block's output, already
    ReLU-masked.  The two 64->256 convolutions (conv3, downsample) and their BatchNorms run in linear form:
    sums, weight gradient and data gradient come from v^T a, a^T a, sum a, sum v, so no 256-channel conv
    output is read in the backward (``head_part``, RoIPool's own sums for the last bn3, is not needed).
    Returns the ReLU-masked gradient w.r.t. the max-pool output (sv['pool_part'] holds the stem's sums), or None when
    ``plan`` (grad_plan) leaves out the "stem" stage.  A 3x3 / conv1 weight whose "wgrad:" stage is left out gets no
    weight-gradient launch (the 3x3 data gradient then reads its operand through the two-tensor prologue)."""
    if plan is None:
        plan = full_plan(params)
    B, H, W, H1, W1, H2, W2 = sv["dims"]
    R = B * H2 * W2
    nt = conv3_num_partials(B, H2, W2)
    ws3 = _empty((query("cova_conv3x3_wgrad4_workspace_floats", B, H2, W2),), g)
    ws1 = _empty((max(query("cova_conv1x1_wgrad_workspace_floats", R, C256, C64),
                      query("cova_conv1x1_vprod_workspace_floats", R)),), g)
    nd = query("cova_conv1x1_lin_dgrad_num_partials", R)
    stem = sv["bn1"]
    for blk in (2, 1, 0):
        s = sv["blocks"][blk]
        pre, cin, bn1, bn2, bn3 = s["pre"], s["cin"], s["bn1"], s["bn2"], s["bn3"]
        w1, w3 = params[pre + "conv1.weight"], params[pre + "conv3.weight"]
        # conv3 (64->256) + bn3; its input a2 = relu(bn2(z2)) on load, bn2's ReLU mask + sums in the epilogue
        avec, m3, cvec = _lin_conv_bn_bwd(g, s["z2"], bn2.abc, 1, w3, bn3, R, gout, pre + "bn3.",
                                          pre + "conv3.weight", grads, ws1)
        part = _empty((nd, 2, C64), g)
        dy2 = _empty((B, H2, W2, C64), g)
        call("cova_conv1x1_lin_dgrad", g, avec, w3, s["z2"], bn2.abc, 1, m3, cvec, None, bn2.scale, bn2.shift,
             s["z2"], bn2.mean, bn2.invstd, dy2, part, R)
        dg, db, abc2 = _bn_abc_from_partials(part, nd, bn2, R, gout, pre + "bn2.", g)
        grads[pre + "bn2.weight"], grads[pre + "bn2.bias"] = dg, db
        # conv2 (3x3): Winograd weight / data gradient, bn1's ReLU mask + sums in the epilogue
        if "wgrad:" + pre + "conv2.weight" in plan:
            dw = _gbuf(gout, pre + "conv2.weight", (C64, C64, 3, 3), g)
            # ... with dz2 = abc2 . (dy2, z2) as its side output: the data gradient below reads one tensor, no prologue
            dzm = _empty((B, H2, W2, C64), g)
            call("cova_conv3x3_wgrad4_partial", s["z1"], bn1.abc, 1, dy2, s["z2"], abc2, dzm, ws3, B, H2, W2)
            call("cova_conv3x3_wgrad4_finish", ws3, dw, None, None, None, None, None, None, B, H2, W2)
            d_in, d_in2, d_abc = dzm, None, None
            grads[pre + "conv2.weight"] = dw
        else:
            d_in, d_in2, d_abc = dy2, s["z2"], abc2
        dy1 = _empty((B, H2, W2, C64), g)
        part = _empty((nt, 2, C64), g)
        dg, db, abc1 = dgrad_bn_bwd(s["ud"], d_in, d_in2, d_abc, None, None, bn1.scale, bn1.shift, s["z1"], bn1, dy1, part,
                                    nt, R, gout, pre + "bn1.", B, H2, W2)
        grads[pre + "bn1.weight"], grads[pre + "bn1.bias"] = dg, db
        # conv1 (Cin->64): dz1 = abc1 . (dy1, z1) on load
        if "wgrad:" + pre + "conv1.weight" in plan:
            dw = _gbuf(gout, pre + "conv1.weight", (C64, cin, 1, 1), g)
            call("cova_conv1x1_wgrad", dy1, s["z1"], abc1, s["x"], None, 0, dw, ws1, R, C64, cin)
            grads[pre + "conv1.weight"] = dw
        if blk > 0:
            # gradient w.r.t. the previous block's output = conv1's data gradient + the identity branch,
            # masked by that output's ReLU (its BatchNorm sums are taken by the next iteration's v^T a)
            dx = _empty((B, H2, W2, C256), g)
            if s.get("x_bits") is not None:
                conv1x1(dy1, s["z1"], abc1, 0, w1, 1, dx, None, R, C64, C256, addend=g, act_bits=s["x_bits"])
            else:
                conv1x1(dy1, s["z1"], abc1, 0, w1, 1, dx, None, R, C64, C256, addend=g, act=s["x"])
            g = dx
        else:
            # downsample branch (64->256 conv + BatchNorm on the block input p1), linear form as well; then
            # dp1 = conv1's + the downsample conv's data gradients, the stem's ReLU mask (from the pooled
            # arg-max pre-activation) and BatchNorm sums
            wdn = params[pre + "downsample.0.weight"]
            avd, md, cvd = _lin_conv_bn_bwd(g, s["x"], None, 0, wdn, s["bnd"], R, gout, pre + "downsample.1.",
                                            pre + "downsample.0.weight", grads, ws1)
            if "stem" not in plan:
                return None
            t = _empty((B, H2, W2, C64), g)
            conv1x1(dy1, s["z1"], abc1, 0, w1, 1, t, None, R, C64, C64)
            sv["pool_part"], sv["pool_npart"] = _empty((nd, 2, C64), g), nd
            dp = _empty((B, H2, W2, C64), g)
            call("cova_conv1x1_lin_dgrad", g, avd, wdn, s["x"], _ident_abc(g), 0, md, cvd, t, stem.scale,
                 stem.shift, sv["ymax"], stem.mean, stem.invstd, dp, sv["pool_part"], R)
            g = dp
    return g


def block_a1(blk):
    """a1 = relu(bn1(z1)) of a BasicBlock; materialised on demand when the fused path skipped it
    (same fma expression as the conv prologue, so ReLU decisions are identical)."""
    if blk["a1"] is not None:
        return blk["a1"]
    z1, bna = blk["z1"], blk["bna"]
    a1 = torch.empty_like(z1)
    call("cova_bn_act_fwd", z1, C64, bna.scale, bna.shift, None, 0, a1, C64, z1.numel() // C64, C64, 1)
    return a1


def block_out(blk):
    """out = relu(bn2(z2) + x) of a BasicBlock; materialised on demand when the forward left it lazy."""
    if blk["out"] is not None:
        return blk["out"]
    z2, bnb = blk["z2"], blk["bnb"]
    out = torch.empty_like(z2)
    call("cova_bn_act_fwd", z2, C64, bnb.scale, bnb.shift, blk["x"], C64, out, C64, z2.numel() // C64, C64, 1)
    return out


def bn_bwd_from_partials(part, nparts, dy, z, st, R, dz, gout, prefix):
    """Finalize + apply when the (sum dy, sum dy*xhat) partials were produced by a fused conv
    epilogue and ``dy`` is already ReLU-masked."""
    C = st.C
    dgamma = _gbuf(gout, prefix + "weight", (C,), z)
    dbeta = _gbuf(gout, prefix + "bias", (C,), z)
    coef = bn_finalize_bwd(part, nparts, C, R, dgamma, dbeta, "pages", frozen=st.frozen)
    call("cova_bn_bwd_apply", dy, C, None, 0, z, C, st.mean, st.invstd, st.scale, coef, dz, C, None, 0,
         R, C)
    return dgamma, dbeta


def dgrad_bn_bwd(u, g_in, g_in2, g_abc, addend, act, msc, msh, z, st, out, part, nt, count, gout, prefix, B, H, W,
                 act_bits=None):
    """Data-gradient conv3x3 (input g_abc . (g_in, g_in2) on load, + addend) whose epilogue masks with the ReLU of
    BatchNorm `st` and takes its backward sums; -> (dgamma, dbeta, abc) of that BatchNorm (finalized by the launch's tail
    or by a separate cova_bn_finalize_bwd_abc).  ``count`` = elements per channel of that BatchNorm."""
    if tails_on() and not st.frozen:
        dg, db, abc, tail = bn_tail_bwd(st, count, gout, prefix, out)
        conv3x3_pro(u, g_in, g_in2, g_abc, 0, addend, act, msc, msh, z, st.mean, st.invstd, out, part, B, H, W, tail,
                    act_bits=act_bits)
        return dg, db, abc
    conv3x3_pro(u, g_in, g_in2, g_abc, 0, addend, act, msc, msh, z, st.mean, st.invstd, out, part, B, H, W)
    C = st.C
    dg = _gbuf(gout, prefix + "weight", (C,), out)
    db = _gbuf(gout, prefix + "bias", (C,), out)
    abc = bn_finalize_bwd(part, nt, C, count, dg, db, "pages", abc_from=st, frozen=st.frozen)
    return dg, db, abc


def _bn_abc_from_partials(part, nparts, st, R, gout, prefix, like):
    """(dgamma, dbeta, abc) with dz = abc[0]*dy + abc[1]*z + abc[2] (applied on load downstream)."""
    C = st.C
    dgamma = _gbuf(gout, prefix + "weight", (C,), like)
    dbeta = _gbuf(gout, prefix + "bias", (C,), like)
    abc = bn_finalize_bwd(part, nparts, C, R, dgamma, dbeta, "pages", abc_from=st, frozen=st.frozen)
    return dgamma, dbeta, abc


def _layer1_bwd_fused(sv, dfeat, gout, grads, head_part=None, plan=None):
    """Backward of the two BasicBlocks with every BatchNorm-backward apply (except the one fed by
    RoIPool's scatter) and both a1 = relu(bn1(z1)) recomputations folded into the Winograd kernels.
    Returns the gradient w.r.t. the max-pool output; sv['pool_abc'] = (dgamma, dbeta, abc) of the stem's BatchNorm.
    ``plan`` (grad_plan; None = everything): a 3x3 weight without its "wgrad:" stage gets no partial launch (its finish
    slot is empty, the data gradient that follows reads its operand through the two-tensor prologue); without "stem"
    block 0's conv1 data gradient is not issued and None is returned."""
    if plan is None:
        plan = frozenset(["stem"] + ["wgrad:%s.weight" % k for k in CONV3_KEYS])
    B, H, W, H1, W1, H2, W2 = sv["dims"]
    R = B * H2 * W2
    # weight gradients: the four launches leave their per-block partial sums in four workspaces, ONE launch at the end
    # folds and transforms them (4 x 67 MB at configs[1]; a shared workspace would need a finish launch per convolution)
    wg = "cova_conv3x3_wgrad4"
    nws = query("cova_conv3x3_wgrad4_workspace_floats", B, H2, W2)
    wanted = [k for k in CONV3_KEYS if "wgrad:%s.weight" % k in plan]
    ws_all = _empty((len(wanted), nws), dfeat) if wanted else None
    jobs = {}               # finish slot (launch order: block 1 conv2, conv1, block 0 conv2, conv1) -> (workspace, dw)

    def wgrad(key, act, act_abc, act_relu, dz, dz2, dz_abc, side=True):
        """-> the gradient operand dz_abc . (dz, dz2) as a materialised map (F(4x4) kernel's side output) or None;
        nothing is launched for a weight outside the plan"""
        if key not in wanted:
            return None
        dw = _gbuf(gout, key + ".weight", (64, 64, 3, 3), dfeat)
        out = torch.empty_like(dz) if dz_abc is not None and side else None
        ws = ws_all[len(jobs)]
        call(wg + "_partial", act, act_abc, act_relu, dz, dz2, dz_abc, out, ws, B, H2, W2)
        jobs[3 - CONV3_KEYS.index(key)] = (ws, dw)
        grads[key + ".weight"] = dw
        return out

    nt = conv3_num_partials(B, H2, W2)
    # head_part = (partials, count): dfeat is already ReLU-masked and the BatchNorm-backward sums of
    # the last bn2 were taken by cova_roipool_bwd_bn
    dA, pend = dfeat, None                  # pend = (dgamma, dbeta, abc) of the bn2 in front of dA, when already known
    if isinstance(head_part, dict):
        pend = head_part["pend"]
    elif head_part is not None:
        last = sv["blocks"][1]["bnb"]
        pend = _bn_abc_from_partials(head_part[0], head_part[1], last, R, gout, BN3_KEYS[3], dfeat)
    for blk in (1, 0):
        s = sv["blocks"][blk]
        ka, kb = CONV3_KEYS[2 * blk], CONV3_KEYS[2 * blk + 1]
        pa, pb = BN3_KEYS[2 * blk], BN3_KEYS[2 * blk + 1]
        bna, bnb = s["bna"], s["bnb"]
        # ---- out = relu(bn2(z2) + x): dz2 = abc_b . (dres, z2); dres = masked incoming gradient
        if pend is None:
            dres, dz2 = torch.empty_like(dA), torch.empty_like(dA)
            dg, db = bn_backward(dA, C64, block_out(s), C64, s["z2"], C64, bnb, R, dz2, C64, dres, C64,
                                 gout, pb, unit="pages")
            g_in, g_in2, g_abc = dz2, None, None
        else:
            dres = dA
            dg, db, g_abc = pend
            g_in, g_in2 = dA, s["z2"]
        grads[pb + "weight"], grads[pb + "bias"] = dg, db
        dzm = wgrad(kb, s["z1"], bna.abc, 1, g_in, g_in2, g_abc)
        if dzm is not None:             # the data gradient below reads the materialised operand: one tensor, no prologue
            g_in, g_in2, g_abc = dzm, None, None
        # ---- dgrad of conv2 with bn1's ReLU mask (recomputed from z1) + backward sums in the epilogue
        dy_a = torch.empty_like(dA)
        part = _empty((nt, 2, C64), dfeat)
        dg, db, abc_a = dgrad_bn_bwd(sv["wd"][2 * blk + 1], g_in, g_in2, g_abc, None, None, bna.scale, bna.shift, s["z1"],
                                     bna, dy_a, part, nt, R, gout, pa, B, H2, W2)
        grads[pa + "weight"], grads[pa + "bias"] = dg, db
        last_dgrad = blk == 1 or "stem" in plan         # (block 0's conv1 data gradient: only for the stem's backward)
        dzm = wgrad(ka, s["x"], None, 0, dy_a, s["z1"], abc_a, side=last_dgrad)
        if not last_dgrad:
            dA = None
            break
        d_in, d_in2, d_abc = (dy_a, s["z1"], abc_a) if dzm is None else (dzm, None, None)
        # ---- dgrad of conv1 (+ residual gradient); for block 1 the epilogue prepares block 0's bn2
        dx = torch.empty_like(dA)
        if blk == 1:
            prev = sv["blocks"][0]
            pend = dgrad_bn_bwd(sv["wd"][2 * blk], d_in, d_in2, d_abc, dres, prev["out"], None, None, prev["z2"],
                                prev["bnb"], dx, _empty((nt, 2, C64), dfeat), nt, R, gout, BN3_KEYS[1], B, H2, W2,
                                act_bits=prev.get("out_bits"))
        elif sv.get("ymax") is not None:
            # stem: ReLU mask of bn1 (from the pooled arg-max value) + its backward sums in the epilogue
            bn1 = sv["bn1"]
            sv["pool_abc"] = dgrad_bn_bwd(sv["wd"][2 * blk], d_in, d_in2, d_abc, dres, None, bn1.scale, bn1.shift,
                                          sv["ymax"], bn1, dx, _empty((nt, 2, C64), dfeat), nt, B * H1 * W1, gout,
                                          "convnet.1.", B, H2, W2)
        else:
            conv3x3_pro(sv["wd"][2 * blk], d_in, d_in2, d_abc, 0, dres, None, None, None, None, None, None, dx,
                        None, B, H2, W2)
        dA = dx
    if jobs:
        fin = []
        for i in range(4):
            fin += list(jobs.get(i, (None, None)))
        call(wg + "_finish", *fin, B, H2, W2)
    return dA


# ---- optional layer2 stage (backbone_layers=2: torchvision resnet18 children()[:-4]): two BasicBlocks 64 -> 128 channels,
# block 0 at stride 2 with the 1x1 stride-2 downsample.  Convolutions: the channel-generic NHWC kernels of
# csrc/conv_nhwc.hip; BatchNorm: the channel-generic statistics / finalize / apply kernels (cova_colstats,
# cova_bn_finalize_*, cova_bn_act(2)_fwd, cova_bn_bwd_reduce / _apply), so SyncBN exchanges their rows like any other.
C128 = 2 * C64
L2 = "convnet.5."
# (state_dict key, Ci, k, stride, pad) of the five convolutions, in forward order
L2_CONVS = [(L2 + "0.conv1", C64, 3, 2, 1), (L2 + "0.conv2", C128, 3, 1, 1), (L2 + "0.downsample.0", C64, 1, 2, 0),
            (L2 + "1.conv1", C128, 3, 1, 1), (L2 + "1.conv2", C128, 3, 1, 1)]


def conv_nhwc_prep(w, fwd=True, dgrad=True):
    """OIHW weight -> (forward operand, data-gradient operand) of the NHWC kernels (either None when not asked for)."""
    co, ci, k, _ = w.shape
    wf = _empty((k * k * ci, co), w) if fwd else None
    wd = _empty((k * k * co, ci), w) if dgrad else None
    call("cova_conv_nhwc_prep", w, wf, wd, co, ci, k)
    return wf, wd


def _layer2_fwd(x, params, buffers, training, save, sv):
    """layer1's output x [B,H2,W2,64] -> layer2's output [B,H3,W3,128]; sv["layer2"] keeps what _layer2_bwd needs."""
    B, H2, W2, _ = x.shape
    H3, W3 = query("cova_conv_out_size", H2, 3, 2, 1), query("cova_conv_out_size", W2, 3, 2, 1)
    R = B * H3 * W3
    ops = {key: conv_nhwc_prep(params[key + ".weight"], dgrad=save) for key, *_ in L2_CONVS}
    geo = {key: rest for key, *rest in L2_CONVS}

    def conv(inp, key):
        ci, k, s, p = geo[key]
        out = _empty((B, H3, W3, C128), x)
        call("cova_conv_nhwc_fwd", inp, ops[key][0], out, B, inp.shape[1], inp.shape[2], ci, C128, k, s, p)
        return out

    def bn(z, prefix):
        if is_train(training, prefix):
            part, n = colstats(z, C128, R, C128)
            return bn_params(prefix, params, buffers, C128, z, training, part, n, R, unit="pages")
        return bn_params(prefix, params, buffers, C128, z, training)

    z1 = conv(x, L2 + "0.conv1")
    s1 = bn(z1, L2 + "0.bn1.")
    a1 = bn_act(z1, s1)
    z2 = conv(a1, L2 + "0.conv2")
    s2 = bn(z2, L2 + "0.bn2.")
    zd = conv(x, L2 + "0.downsample.0")
    sd = bn(zd, L2 + "0.downsample.1.")
    out0 = _empty((B, H3, W3, C128), x)
    call("cova_bn_act2_fwd", z2, s2.scale, s2.shift, zd, sd.scale, sd.shift, out0, R, C128, 1)
    z3 = conv(out0, L2 + "1.conv1")
    s3 = bn(z3, L2 + "1.bn1.")
    a3 = bn_act(z3, s3)
    z4 = conv(a3, L2 + "1.conv2")
    s4 = bn(z4, L2 + "1.bn2.")
    out1 = bn_act(z4, s4, res=out0)
    if save:
        sv["layer2"] = dict(dims=(B, H2, W2, H3, W3), wd={k: v[1] for k, v in ops.items()}, x=x, z1=z1, s1=s1, a1=a1,
                            z2=z2, s2=s2, zd=zd, sd=sd, out0=out0, z3=z3, s3=s3, a3=a3, z4=z4, s4=s4, out1=out1)
    return out1


def _layer2_bwd(s, g, gout, grads, plan=None):
    """g = dL/d(layer2's output), not yet ReLU-masked -> dL/d(layer1's output) (None when the plan has no "layer1"
    stage: block 0's two data gradients are then not launched).  Weight gradients only for the plan's "wgrad:" keys."""
    B, H2, W2, H3, W3 = s["dims"]
    R = B * H3 * W3
    geo = {key: rest for key, *rest in L2_CONVS}

    def wgrad(inp, dz, key):
        if plan is not None and "wgrad:%s.weight" % key not in plan:
            return
        ci, k, st, p = geo[key]
        dw = _gbuf(gout, key + ".weight", (C128, ci, k, k), g)
        ws = _empty((query("cova_conv_nhwc_wgrad_workspace_floats", B, H3, W3, ci, C128, k),), g)
        call("cova_conv_nhwc_wgrad", inp, dz, dw, ws, B, inp.shape[1], inp.shape[2], ci, C128, k, st, p)
        grads[key + ".weight"] = dw

    def dgrad(dz, key, addend=None):
        dx = torch.empty_like(dz)
        call("cova_conv_nhwc_dgrad", dz, s["wd"][key], None, None, addend, dx, B, H3, W3, C128, C128, 3, 1, 1)
        return dx

    def bnb(dout, act, z, st, prefix, dres=None):
        dz = torch.empty_like(z)
        dg, db = bn_backward(dout, C128, act, C128, z, C128, st, R, dz, C128, dres, C128 if dres is not None else 0,
                             gout, prefix, unit="pages")
        grads[prefix + "weight"], grads[prefix + "bias"] = dg, db
        return dz

    # block 1: out1 = relu(bn2(z4) + out0), z4 = conv2(a3), a3 = relu(bn1(z3)), z3 = conv1(out0)
    gres = torch.empty_like(g)
    dz4 = bnb(g, s["out1"], s["z4"], s["s4"], L2 + "1.bn2.", dres=gres)
    wgrad(s["a3"], dz4, L2 + "1.conv2")
    dz3 = bnb(dgrad(dz4, L2 + "1.conv2"), s["a3"], s["z3"], s["s3"], L2 + "1.bn1.")
    wgrad(s["out0"], dz3, L2 + "1.conv1")
    dout0 = dgrad(dz3, L2 + "1.conv1", addend=gres)
    # block 0: out0 = relu(bn2(z2) + bnd(zd)), z2 = conv2(a1), a1 = relu(bn1(z1)), z1 = conv1(x), zd = downsample(x)
    gres0 = torch.empty_like(g)
    dz2 = bnb(dout0, s["out0"], s["z2"], s["s2"], L2 + "0.bn2.", dres=gres0)
    dzd = bnb(gres0, None, s["zd"], s["sd"], L2 + "0.downsample.1.")
    wgrad(s["a1"], dz2, L2 + "0.conv2")
    wgrad(s["x"], dzd, L2 + "0.downsample.0")
    dz1 = bnb(dgrad(dz2, L2 + "0.conv2"), s["a1"], s["z1"], s["s1"], L2 + "0.bn1.")
    wgrad(s["x"], dz1, L2 + "0.conv1")
    if plan is not None and "layer1" not in plan:
        return None
    # both stride-2 data gradients land on layer1's output: one launch, the downsample's as one more tap
    dx = torch.empty_like(s["x"])
    call("cova_conv_nhwc_dgrad", dz1, s["wd"][L2 + "0.conv1"], dzd, s["wd"][L2 + "0.downsample.0"], None, dx,
         B, H2, W2, C64, C128, 3, 2, 1)
    return dx


def masked_grad_and_sums(dout, last, R):
    """Stand-alone form of what cova_roipool_bwd_bn fuses: g = dout * (out > 0) and the partial rows of
    (sum g, sum g*xhat(z)) for the BatchNorm in front of the feature map."""
    st, z = last["bn"], last["z"]
    C = st.C
    out = last["out"] if last["out"] is not None else bn_act(z, st, last["x"])
    n = query("cova_colreduce_num_chunks", R, C)
    part = _empty((n, 2, C), z)
    call("cova_bn_bwd_reduce", dout, C, out, C, z, C, st.mean, st.invstd, R, C, part)
    g = torch.empty_like(dout)
    zero = torch.zeros((2, C), device=z.device)
    # coef = 0 and scale = 1 turn the apply kernel into the plain ReLU mask: dres = dout * (out > 0)
    call("cova_bn_bwd_apply", dout, C, out, C, z, C, st.mean, st.invstd, torch.ones_like(st.scale), zero,
         torch.empty_like(dout), C, g, C, R, C)
    return g, (part, n)


@on_device_of(1)
def convstack_bwd(sv, dfeat, gout=None, head_part=None, params=None, want_dimg=False, plan=None):
    """dfeat NHWC [B,Hf,Wf,C] -> {state_dict key: grad} for the convs and BatchNorms of the stack; with ``want_dimg`` also
    the gradient w.r.t. the images (NCHW) under the key "__images__" (needs ``params``: conv1's weight).

    The data-gradient convs carry the ReLU mask and the BatchNorm-backward reduction of the layer
    in front of them in their epilogue (and its finalize in their tail), so only the last block's bn2
    (whose incoming gradient is RoIPool's scatter) needs a stand-alone reduction / finalize.
    ``params`` is needed by the resnet50 extension (its 1x1 convs read the weights directly) and by ``want_dimg``
    (conv1's weight).  ``plan`` (grad_plan; None = every gradient): the stages it leaves out are not launched and their
    gradients are absent from the result."""
    if want_dimg and (params is None or "convnet.0.weight" not in params):
        raise ValueError("convstack_bwd(want_dimg=True) needs params with 'convnet.0.weight' (the transposed conv1)")
    if sv["kind"] == "bottleneck" and params is None:
        raise ValueError("convstack_bwd of the resnet50 stack needs params (its 1x1 convolutions read the weights)")
    B, H, W, H1, W1, H2, W2 = sv["dims"]
    R = B * H2 * W2
    grads = {}
    if plan is not None and want_dimg:
        plan = plan | {"stem", "layer1"}
    if sv.get("layer2") is not None:
        dfeat = _layer2_bwd(sv["layer2"], dfeat, gout, grads, plan)
        if dfeat is None:               # the plan ends at layer2 (layer1 and the stem frozen, no image gradient)
            return grads
        head_part = None
    if sv["kind"] == "bottleneck":
        if head_part is None:          # piecewise API (_get_visual_features): mask + sums stand-alone
            dfeat, head_part = masked_grad_and_sums(dfeat, sv["last"], R)
        dA = _layer1_bottleneck_bwd(sv, dfeat, params, gout, grads, head_part, plan)
    else:
        dA = _layer1_bwd_fused(sv, dfeat, gout, grads, head_part, plan)
    if dA is None:                      # the plan ends at layer1 (stem frozen, no image gradient)
        return grads
    # maxpool + relu + bn1, then conv1's weight gradient
    bn1 = sv["bn1"]
    wgrad1 = plan is None or "conv1_wgrad" in plan
    ws1 = _empty((query("cova_conv1_wgrad_workspace_floats", B, H, W),), dfeat) if wgrad1 else None
    dw1 = _gbuf(gout, "convnet.0.weight", (64, 3, 7, 7), dfeat) if wgrad1 else None
    pool_abc = sv.get("pool_abc")
    if pool_abc is None and sv.get("pool_part") is not None:        # (resnet50 stack: its last launch left the partials)
        dg = _gbuf(gout, "convnet.1.weight", (C64,), dfeat)
        db = _gbuf(gout, "convnet.1.bias", (C64,), dfeat)
        pool_abc = (dg, db, bn_finalize_bwd(sv["pool_part"], sv["pool_npart"], C64, B * H1 * W1, dg, db, "pages",
                                            abc_from=bn1, frozen=bn1.frozen))
    if pool_abc is not None:
        # dA is already ReLU-masked (epilogue of the last data-gradient conv): the pooling/BN backward
        # apply is folded into conv1's weight-gradient kernel, dy1 is never written
        dg, db, abc = pool_abc
        if wgrad1:
            call("cova_conv1_wgrad_poolbwd", sv["images"], sv["y1"], dA, sv["idx"], abc, dw1, ws1, B, H, W)
        if want_dimg:                   # images.requires_grad: dy1 written out once, then the transposed convolution
            dy1 = torch.empty_like(sv["y1"])
            call("cova_pool_bwd_dy1", dA, sv["idx"], sv["y1"], abc, dy1, B, H1, W1)
    else:
        npart = query("cova_bn_relu_maxpool_bwd_num_partials", B, H1, W1)
        part = _empty((npart, 2, C64), dfeat)
        call("cova_bn_relu_maxpool_bwd_reduce", dA, sv["idx"], sv["y1"], bn1.scale, bn1.shift, bn1.mean,
             bn1.invstd, part, B, H1, W1)
        dg = _gbuf(gout, "convnet.1.weight", (C64,), dfeat)
        db = _gbuf(gout, "convnet.1.bias", (C64,), dfeat)
        coef = bn_finalize_bwd(part, npart, C64, B * H1 * W1, dg, db, "pages", frozen=bn1.frozen)
        if wgrad1 or want_dimg:
            dy1 = torch.empty_like(sv["y1"])
            call("cova_bn_relu_maxpool_bwd_apply", dA, sv["idx"], sv["y1"], bn1.scale, bn1.shift, bn1.mean,
                 bn1.invstd, coef, dy1, B, H1, W1)
        if wgrad1:
            call("cova_conv1_wgrad", sv["images"], dy1, dw1, ws1, B, H, W)
    grads["convnet.1.weight"], grads["convnet.1.bias"] = dg, db
    if wgrad1:
        grads["convnet.0.weight"] = dw1
    if want_dimg:
        dimg = torch.empty_like(sv["images"])
        call("cova_conv1_dgrad", dy1, params["convnet.0.weight"], dimg, B, H, W)
        grads["__images__"] = dimg
    return grads


# ------------------------------------------------------------------------------- RoIPool
def roipool_fwd(feat, bboxes, roi_size, spatial_scale, out, ld_out):
    """feat: NHWC tensor or a LazyFeature (then bn2 + residual + ReLU are formed inside the kernel)."""
    _check(bboxes)
    B, Hf, Wf, C = feat.shape
    N = bboxes.shape[0]
    PH, PW = roi_size
    argmax = _empty((N, C * PH * PW), bboxes, torch.int32)
    zmax = None
    if isinstance(feat, LazyFeature):
        zmax = _empty((N, C * PH * PW), bboxes)
        call("cova_roipool_fwd_bn", feat.z, feat.x, feat.scale, feat.shift, bboxes, N, B, C, Hf, Wf, PH, PW,
             float(spatial_scale), out, ld_out, argmax, zmax)
    else:
        call("cova_roipool_fwd", feat, bboxes, N, B, C, Hf, Wf, PH, PW, float(spatial_scale), out, ld_out,
             argmax)
    return dict(argmax=argmax, bboxes=bboxes, shape=(B, Hf, Wf, C), roi=(PH, PW), scale=float(spatial_scale),
                zmax=zmax, pooled=out, ld_pooled=ld_out)


def roialign_fwd(feat, bboxes, roi_size, spatial_scale, sampling_ratio, aligned, out, ld_out):
    """RoIAlign variant of the pooling stage (extension: north_star names RoIAlign, the reference uses RoIPool)."""
    _check(bboxes)
    B, Hf, Wf, C = feat.shape
    N = bboxes.shape[0]
    PH, PW = roi_size
    call("cova_roialign_fwd", feat, bboxes, N, B, C, Hf, Wf, PH, PW, float(spatial_scale), int(sampling_ratio),
         1 if aligned else 0, out, ld_out)
    return dict(kind="align", bboxes=bboxes, shape=(B, Hf, Wf, C), roi=(PH, PW), scale=float(spatial_scale),
                sampling_ratio=int(sampling_ratio), aligned=bool(aligned), zmax=None)


def roialign_bwd(sv, gout, ld_g):
    B, Hf, Wf, C = sv["shape"]
    PH, PW = sv["roi"]
    gfeat = _empty((B, Hf, Wf, C), gout)
    call("cova_roialign_bwd", gout, ld_g, sv["bboxes"], sv["bboxes"].shape[0], B, C, Hf, Wf, PH, PW, sv["scale"],
         sv["sampling_ratio"], 1 if sv["aligned"] else 0, gfeat, _empty((2 * B + 16,), gout, torch.int32))
    return gfeat


def _roipool_ws(sv, like):
    B, Hf, Wf, C = sv["shape"]
    PH, PW = sv["roi"]
    return _empty((query("cova_roipool_bwd_workspace_words", sv["bboxes"].shape[0], B, C, PH, PW),), like, torch.int32)


def roipool_bwd(sv, gout, ld_g):
    B, Hf, Wf, C = sv["shape"]
    PH, PW = sv["roi"]
    gfeat = _empty((B, Hf, Wf, C), gout)
    call("cova_roipool_bwd", gout, ld_g, sv["bboxes"], sv["argmax"], sv["bboxes"].shape[0], B, C, Hf,
         Wf, PH, PW, float(sv["scale"]), gfeat, _roipool_ws(sv, gout))
    return gfeat


def roipool_bwd_bn(sv, gout, ld_g, last, grad_out=None):
    """RoIPool backward for the un-materialised feature map relu(bn(z) + x): the ReLU mask is `pooled > 0`
    (the pooled value is the map's value at the arg-max) and the BatchNorm-backward sums are taken per
    pooled entry from the z values the forward kept -> (masked gradient map, (partials, count)), or -- 64-channel
    stack, BatchNorm tails on -- (map, {"pend": (dgamma, dbeta, abc)}) with that BatchNorm's finalize done by the
    entry pass's last block."""
    B, Hf, Wf, C = sv["shape"]
    PH, PW = sv["roi"]
    n = sv["bboxes"].shape[0]
    gfeat = _empty((B, Hf, Wf, C), gout)
    npart = query("cova_roipool_bwd_bn_num_partials", n)
    part = _empty((npart, 2, C), gout)
    bn = last["bn"]
    if tails_on(C) and not bn.frozen and last.get("prefix"):
        dg, db, abc, tail = bn_tail_bwd(bn, B * Hf * Wf, grad_out, last["prefix"], gout)
        call("cova_roipool_bwd_bn_tail", gout, ld_g, sv["pooled"], sv["ld_pooled"], sv["zmax"], sv["bboxes"],
             sv["argmax"], n, B, C, Hf, Wf, PH, PW, float(sv["scale"]), bn.mean, bn.invstd, gfeat, part,
             _roipool_ws(sv, gout), tail.ptr)
        return gfeat, {"pend": (dg, db, abc)}
    call("cova_roipool_bwd_bn", gout, ld_g, sv["pooled"], sv["ld_pooled"], sv["zmax"], sv["bboxes"], sv["argmax"],
         n, B, C, Hf, Wf, PH, PW, float(sv["scale"]), bn.mean, bn.invstd, gfeat, part, _roipool_ws(sv, gout))
    return gfeat, (part, npart)


# ------------------------------------------------------------------------------- BN over [N, C]
def bn1d_fused(training):
    """one launch per BatchNorm1d application (csrc/bn1d.hip): train mode without SyncBN"""
    return OPTIONS.bn_tail and training and STAT_SYNC is None


def bn1d_fwd(x, ldx, N, C, prefix, params, buffers, training, out, ldo, relu, drop=None):
    """BatchNorm1d (+ReLU) of x [N,C] into out.  ``drop`` = (p, seed, mask or None): also the Dropout of the result
    -> returns (BNState, dropped, mask).  ``training``: bool or per-layer modes (resolved for ``prefix``)."""
    training = is_train(training, prefix)
    if bn1d_fused(training) and N > 0:
        st = bn_state(C, x, N, True)
        dropped = mask = None
        p, seed, given = 0.0, 0, False
        if drop is not None:
            p, seed, mask = drop
            given = mask is not None
            if given:
                _check(mask, torch.uint8)
            else:
                mask = _empty((N, C), x, torch.uint8)
            dropped = _empty((N, C), x)
        call("cova_bn1d_fwd", x, ldx, N, C, params[prefix + "weight"], params[prefix + "bias"],
             buffers[prefix + "running_mean"], buffers[prefix + "running_var"],
             buffers.get(prefix + "num_batches_tracked"), BN_MOMENTUM, BN_EPS, 1 if relu else 0, out, ldo, dropped, C,
             mask, float(p), int(seed), 1 if given else 0, st.scale, st.shift, st.mean, st.invstd)
        return (st, dropped, mask) if drop is not None else st
    part, n = colstats(x, ldx, N, C) if training else (None, 0)
    st = bn_params(prefix, params, buffers, C, x, training, part, n, N)
    call("cova_bn_act_fwd", x, ldx, st.scale, st.shift, None, 0, out, ldo, N, C, 1 if relu else 0)
    if drop is not None:
        dropped, mask = dropout_fwd(out, ldo, N, C, drop[0], drop[1], drop[2])
        return st, dropped, mask
    return st


# ------------------------------------------------------------------------------- positional encoder
def bbox_fwd(bboxes, params, buffers, training, out, ldo):
    """models.py:129-148: [x1,y1,w,h,w/h] -> Linear(5,Hd) -> BatchNorm1d -> ReLU, written to out."""
    N = bboxes.shape[0]
    Hd = params["bbox_feat_encoder.0.weight"].shape[0]
    raw, z = _empty((N, 5), bboxes), _empty((N, Hd), bboxes)
    call("cova_bbox_linear_fwd", bboxes, params["bbox_feat_encoder.0.weight"],
         params["bbox_feat_encoder.0.bias"], raw, z, N, Hd)
    st = bn1d_fwd(z, Hd, N, Hd, "bbox_feat_encoder.1.", params, buffers, training, out, ldo, True)
    return dict(raw=raw, z=z, st=st, N=N, Hd=Hd, out=out, ldo=ldo)


def bbox_bwd(sv, g, ldg, gout=None):
    N, Hd = sv["N"], sv["Hd"]
    dz = _empty((N, Hd), g)
    dg, db = bn_backward(g, ldg, sv["out"], sv["ldo"], sv["z"], Hd, sv["st"], N, dz, Hd, None, 0,
                         gout, "bbox_feat_encoder.1.")
    dW = _gbuf(gout, "bbox_feat_encoder.0.weight", (Hd, 5), g)
    dbias = _gbuf(gout, "bbox_feat_encoder.0.bias", (Hd,), g)
    call("cova_bbox_linear_bwd", dz, sv["raw"], dW, dbias, N, Hd)
    return {"bbox_feat_encoder.0.weight": dW, "bbox_feat_encoder.0.bias": dbias,
            "bbox_feat_encoder.1.weight": dg, "bbox_feat_encoder.1.bias": db}


# ------------------------------------------------------------------------------- GAT
def _adjacent(a, b):
    """b starts right where a ends AND both are views of ONE storage (the trainer's flat bucket): [a; b] is one row-major
    matrix.  Two separately allocated tensors that the allocator happened to place back to back do not count: the
    one-GEMM and the two-GEMM forms associate their sums differently (an ulp), and which one a model instance takes
    must not depend on where its parameters landed in memory (found with two instances of the drop-in module built from
    one state_dict: bit-different gradients, tests/test_model_gpu.py::test_gradient_with_respect_to_the_images)."""
    return (a.is_contiguous() and b.is_contiguous() and a.shape[1:] == b.shape[1:] and
            b.data_ptr() == a.data_ptr() + a.numel() * a.element_size() and
            a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr())


def _page_hw(page_size):
    """``page_size`` = (height, width) of the pages in pixels, as ``images.shape[2:]`` -> two positive floats."""
    try:
        H, W = (float(v) for v in page_size)
    except (TypeError, ValueError):
        raise ValueError("page_size must be (height, width) in pixels, got %r" % (page_size,))
    if not (H > 0 and W > 0):
        raise ValueError("page_size must be positive, got %r" % (page_size,))
    return H, W


def edge_geometry(bboxes, ctx, page_size):
    """phi [N, K, 8]: the relative geometry of every edge of the context table (include/cova_hip.h, cova_edge_geometry).
    ``page_size`` = (height, width) of the pages in pixels, as ``images.shape[2:]``.  One launch per batch; every head
    and layer of the GAT stack shares the result."""
    _check(bboxes)
    _check(ctx, torch.int64)
    H, W = _page_hw(page_size)
    N, K = ctx.shape
    phi = _empty((N, K, 8), bboxes)
    call("cova_edge_geometry", bboxes, ctx, N, K, W, H, phi)
    return phi


def check_attention_weight(prefix, aw, D, attention):
    """The mode the caller asks for against the one the head's ``attention_layer.weight`` was built for."""
    from .weights import attention_of, check_attention
    check_attention(attention)
    have = attention_of(aw, D, prefix)
    if have != attention:
        raise ValueError("attention=%r, but %sattention_layer.weight has shape %s: it belongs to attention=%r "
                         "(a 'gat' head scores with [1, %d], a 'gatv2' head with [1, %d])"
                         % (attention, prefix, tuple(aw.shape), have, 2 * D, D))


def dropout_base(seed, call):
    """First dropout stream of forward number ``call`` (1, 2, ...) under ``seed``: CoVA._next_dropout_seeds' and
    HotPathTrainer.forward_backward's rule.  The decoder draws from ``base`` and ``base + 1``; the next call's is ``base + 2``."""
    return (int(seed) * 0x9E3779B1 + 2 * int(call)) & 0xFFFFFFFFFFFF


def attention_dropout_seed(base, layer, head):
    """Stream of the attention dropout of head ``head`` of layer ``layer`` in the step whose decoder Dropouts draw from
    ``base`` and ``base + 1``: ``(layer + 1) << 56 | (head + 1) << 48 | base``.
    Every ``base`` (CoVA._next_dropout_seeds, HotPathTrainer.forward_backward) is below 2**48 and ``base + 1`` at most
    2**48, so the decoder streams of every step and seed have bits 49 .. 63 clear, while an attention stream has one of the
    bits 48 .. 62 set and (head + 1) << 48 | base > 2**48: no attention stream is a decoder stream of any step, and two
    attention streams are equal only for equal (base, layer, head).  The counter hash (csrc/common.h, hash_mix64)
    finalises ``seed + golden * (idx + 1)`` with full avalanche: streams that differ in high bits only are unrelated."""
    base, layer, head = int(base), int(layer), int(head)
    if not (0 <= base < 1 << 48 and 0 <= layer < 127 and 0 <= head < 255):
        raise ValueError("attention_dropout_seed: base in [0, 2**48), layer in [0, 127), head in [0, 255); got %r"
                         % ((base, layer, head),))
    return (layer + 1) << 56 | (head + 1) << 48 | base


PAGE_DROP_SITES = 4         # of an encoder layer: attention probabilities, drop1, the FFN hidden activations, drop2


def page_dropout_seed(base, layer, site):
    """Stream of dropout site ``site`` of page layer ``layer`` in the step whose decoder Dropouts draw from ``base`` and
    ``base + 1``: ``1 << 63 | (layer + 1) << 56 | (site + 1) << 48 | base``.  Encoder layer l is ``layer = l`` with the sites
    0 attention probabilities, 1 drop1 (the attention sublayer's output), 2 the FFN hidden activations, 3 drop2 (the FFN's
    output); the stand-alone page attention is ``layer = weights.PAGE_ENCODER_MAX_LAYERS``, ``site = 0``.
    Every ``base`` is below 2**48 (dropout_base), so the decoder streams ``base`` and ``base + 1`` are at most 2**48, and an
    attention_dropout_seed stream is below 127 << 56 | 255 << 48 | 2**48 < 2**63: bit 63 is clear in all of them and set in
    every page stream, so no page stream is a decoder or a GAT attention stream of any step or seed.  (layer + 1) <= 9 fits
    the bits 56 .. 62 and (site + 1) <= 4 the bits 48 .. 55, so two page streams are equal only for equal (base, layer,
    site).  The counter hash finalises ``seed + golden * (idx + 1)`` with full avalanche (attention_dropout_seed says
    so): streams that differ in high bits only are unrelated."""
    from .weights import PAGE_ENCODER_MAX_LAYERS
    base, layer, site = int(base), int(layer), int(site)
    if not (0 <= base < 1 << 48 and 0 <= layer <= PAGE_ENCODER_MAX_LAYERS and 0 <= site < PAGE_DROP_SITES):
        raise ValueError("page_dropout_seed: base in [0, 2**48), layer in [0, %d], site in [0, %d); got %r"
                         % (PAGE_ENCODER_MAX_LAYERS, PAGE_DROP_SITES, (base, layer, site)))
    return 1 << 63 | (layer + 1) << 56 | (site + 1) << 48 | base


def check_page_drop(drop, option="page dropout"):
    """``drop`` of the page attention core -> (p, seed) with p in (0, 1), or None when there is nothing to drop."""
    if drop is None:
        return None
    from .weights import check_page_dropout
    p, seed = drop
    p, seed = check_page_dropout(p, option), int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("%s seed must fit 64 unsigned bits, got %r" % (option, seed))
    return (p, seed) if p > 0.0 else None


def check_gat_drop(drop):
    """``drop`` of gat_fwd -> (p, seed) with p in (0, 1), or None when there is nothing to drop (None, or p == 0)."""
    if drop is None:
        return None
    from .weights import check_attention_dropout
    p, seed = drop
    p, seed = check_attention_dropout(p), int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("attention dropout seed must fit 64 unsigned bits, got %r" % (seed,))
    return (p, seed) if p > 0.0 else None


def gat_fwd(h, ldh, N, F, ctx, params, hprime, ldo, prefix="gat.", phi=None, attention="gat", drop=None):
    """models.py:171-212.  h rows at h + n*ldh (F values); hprime rows at hprime + n*ldo (D).
    ``phi`` (edge_geometry): the score takes the edge term ``edge_layer.weight . phi`` (cova_gat_fwd_edge); a head that
    has an ``edge_layer.weight`` needs it.
    ``attention="gatv2"``: the score is ``a . LeakyReLU(Wh_i + Wh_j) + b`` (cova_gat2_fwd; the edge term is added outside
    the non-linearity); the projections are the same GEMM(s), and the saved dict carries no ``s`` / ``t``.
    ``drop`` = (p, seed): dropout on the attention coefficients (cova_gat_fwd_drop / cova_gat2_fwd_drop; ``attn`` stays the
    softmax output); None or p == 0 issues exactly the calls above.  gat_bwd reads (p, seed) from the saved dict."""
    _check(ctx, torch.int64)
    drop = check_gat_drop(drop)
    Wi, Wj = params[prefix + "W_i.weight"], params[prefix + "W_j.weight"]
    aw, ab = params[prefix + "attention_layer.weight"], params[prefix + "attention_layer.bias"]
    ew = params.get(prefix + "edge_layer.weight")
    if (ew is None) != (phi is None):
        raise ValueError("%s: %s" % (prefix, "an edge-aware head needs the edge features phi (boxes and page size)"
                                     if phi is None else "edge features given to a head without edge_layer.weight"))
    D, K = Wi.shape[0], ctx.shape[1]
    v2 = attention == "gatv2"
    if aw.shape[-1] != (D if v2 else 2 * D) or not (v2 or attention == "gat"):
        check_attention_weight(prefix, aw, D, attention)          # (raises)
    Wh = _empty((N, 2 * D), h)
    if _adjacent(Wi, Wj):        # one [2D, F] matrix (flat parameter bucket): both projections in one GEMM
        call("cova_sgemm", 0, 1, N, 2 * D, F, h, ldh, Wi, F, Wh, 2 * D, None, 0)
    else:
        call("cova_sgemm", 0, 1, N, D, F, h, ldh, Wi, F, Wh, 2 * D, None, 0)
        call("cova_sgemm", 0, 1, N, D, F, h, ldh, Wj, F, Wh[:, D:], 2 * D, None, 0)
    if v2:
        attn = _empty((N, K), h)
        if phi is not None:
            assert tuple(phi.shape) == (N, K, 8), (tuple(phi.shape), N, K)
            _check(phi), _check(ew)
        if drop is None:
            call("cova_gat2_fwd", Wh, 2 * D, aw, ab, ctx, phi, ew, N, K, D, LEAKY_SLOPE, attn, hprime, ldo)
        else:
            call("cova_gat2_fwd_drop", Wh, 2 * D, aw, ab, ctx, phi, ew, N, K, D, LEAKY_SLOPE, drop[0], drop[1], attn,
                 hprime, ldo)
        return dict(h=h, ldh=ldh, N=N, F=F, D=D, K=K, ctx=ctx, Wh=Wh, attn=attn, prefix=prefix, phi=phi,
                    attention="gatv2", drop=drop)
    s, t, attn = _empty((N,), h), _empty((N,), h), _empty((N, K), h)
    if drop is not None:
        if phi is not None:
            assert tuple(phi.shape) == (N, K, 8), (tuple(phi.shape), N, K)
            _check(phi), _check(ew)
        call("cova_gat_fwd_drop", Wh, 2 * D, aw, ab, ctx, phi, ew, N, K, D, LEAKY_SLOPE, drop[0], drop[1], s, t, attn,
             hprime, ldo)
    elif phi is None:
        call("cova_gat_fwd", Wh, 2 * D, aw, ab, ctx, N, K, D, LEAKY_SLOPE, s, t, attn, hprime, ldo)
    else:
        assert tuple(phi.shape) == (N, K, 8), (tuple(phi.shape), N, K)
        call("cova_gat_fwd_edge", Wh, 2 * D, aw, ab, ctx, _check(phi), _check(ew), N, K, D, LEAKY_SLOPE, s, t, attn,
             hprime, ldo)
    return dict(h=h, ldh=ldh, N=N, F=F, D=D, K=K, ctx=ctx, Wh=Wh, s=s, t=t, attn=attn, prefix=prefix, phi=phi, drop=drop)


# Backward of the neighbour gather: a deterministic gather through the transposed index (no float atomics).
_CSR_WS = {}


def gat_transpose(ctx):
    """Transposed neighbour index of one batch (shared by every head / layer / backward call of the step).  The
    workspace is kept per (device, stream, N, K): its counters are zeroed once and left zero by the kernels.
    The returned tensor IS that cached workspace: it is valid until the next gat_transpose call with the same
    (device, stream, N, K) -- use it within the step that built it (clone it to keep it longer)."""
    N, K = ctx.shape
    key = (ctx.device, torch.cuda.current_stream(ctx.device).cuda_stream, N, K)
    csr = _CSR_WS.get(key)
    if csr is None:
        if len(_CSR_WS) >= 8:
            _CSR_WS.clear()
        csr = _CSR_WS[key] = torch.zeros((query("cova_gat_transpose_ints", N, K),), dtype=torch.int32, device=ctx.device)
    try:
        call("cova_gat_transpose_reuse", ctx, N, K, csr)
    except BaseException:               # (KeyboardInterrupt between the three launches included)
        _CSR_WS.pop(key, None)          # its counters may be half-updated: never reuse it
        raise
    return csr


def gat_bwd(sv, g, ldg, params, dh, lddh, accumulate_dh, gout=None, csr=None):
    """g = dL/dh' (rows at g + n*ldg).  Writes / accumulates dL/dh into dh; returns param grads."""
    N, F, D, K, prefix = sv["N"], sv["F"], sv["D"], sv["K"], sv["prefix"]
    if csr is None:
        csr = gat_transpose(sv["ctx"])
    du = _empty((N, K), g)
    Wi, Wj = params[prefix + "W_i.weight"], params[prefix + "W_j.weight"]
    aw = params[prefix + "attention_layer.weight"]
    dWh = _empty((N, 2 * D), g)
    v2 = sv.get("attention", "gat") == "gatv2"
    if aw.shape[-1] != (D if v2 else 2 * D):
        check_attention_weight(prefix, aw, D, sv.get("attention", "gat"))          # (raises)
    daw = _gbuf(gout, prefix + "attention_layer.weight", (1, D if v2 else 2 * D), g)
    dab = _gbuf(gout, prefix + "attention_layer.bias", (1,), g)
    phi, ew, dew, edge, drop = sv.get("phi"), None, None, {}, sv.get("drop")
    if phi is not None:
        ew = params[prefix + "edge_layer.weight"]
        dew = _gbuf(gout, prefix + "edge_layer.weight", (1, 8), g)
        edge = {prefix + "edge_layer.weight": dew}
    if v2:
        ws = _empty((query("cova_gat2_workspace_floats", N, K, D),), g)
        if drop is None:
            call("cova_gat2_bwd", g, ldg, sv["Wh"], 2 * D, sv["attn"], sv["ctx"], aw, phi, ew, N, K, D, LEAKY_SLOPE, dWh,
                 2 * D, daw, dab, dew, csr, du, ws)
        else:
            call("cova_gat2_bwd_drop", g, ldg, sv["Wh"], 2 * D, sv["attn"], sv["ctx"], aw, phi, ew, N, K, D, LEAKY_SLOPE,
                 drop[0], drop[1], dWh, 2 * D, daw, dab, dew, csr, du, ws)
    else:
        ds, dt = _empty((N,), g), _empty((N,), g)
        if drop is not None:
            ws = _empty((query("cova_gat_edge_workspace_floats", N, K),), g) if phi is not None else None
            call("cova_gat_bwd_drop", g, ldg, sv["Wh"], 2 * D, sv["s"], sv["t"], sv["attn"], sv["ctx"], aw, phi, ew, N, K,
                 D, LEAKY_SLOPE, drop[0], drop[1], dWh, 2 * D, ds, dt, daw, dab, dew, csr, du, ws)
        elif phi is None:
            call("cova_gat_bwd", g, ldg, sv["Wh"], 2 * D, sv["s"], sv["t"], sv["attn"], sv["ctx"], aw, N, K, D,
                 LEAKY_SLOPE, dWh, 2 * D, ds, dt, daw, dab, csr, du)
        else:
            ws = _empty((query("cova_gat_edge_workspace_floats", N, K),), g)
            call("cova_gat_bwd_edge", g, ldg, sv["Wh"], 2 * D, sv["s"], sv["t"], sv["attn"], sv["ctx"], aw, phi, ew, N, K,
                 D, LEAKY_SLOPE, dWh, 2 * D, ds, dt, daw, dab, dew, csr, du, ws)
    dWi = _gbuf(gout, prefix + "W_i.weight", (D, F), g)
    dWj = _gbuf(gout, prefix + "W_j.weight", (D, F), g)
    if _adjacent(dWi, dWj):
        call("cova_sgemm", 1, 0, 2 * D, F, N, dWh, 2 * D, sv["h"], sv["ldh"], dWi, F, None, 0)
    else:
        call("cova_sgemm", 1, 0, D, F, N, dWh, 2 * D, sv["h"], sv["ldh"], dWi, F, None, 0)
        call("cova_sgemm", 1, 0, D, F, N, dWh[:, D:], 2 * D, sv["h"], sv["ldh"], dWj, F, None, 0)
    if _adjacent(Wi, Wj):
        call("cova_sgemm", 0, 0, N, F, 2 * D, dWh, 2 * D, Wi, F, dh, lddh, None, 1 if accumulate_dh else 0)
    else:
        call("cova_sgemm", 0, 0, N, F, D, dWh, 2 * D, Wi, F, dh, lddh, None, 1 if accumulate_dh else 0)
        call("cova_sgemm", 0, 0, N, F, D, dWh[:, D:], 2 * D, Wj, F, dh, lddh, None, 1)
    return dict({prefix + "W_i.weight": dWi, prefix + "W_j.weight": dWj,
                 prefix + "attention_layer.weight": daw, prefix + "attention_layer.bias": dab}, **edge)


def gat_stack_fwd(comb, T, N, F, D, ctx, params, n_heads=1, n_gat_layers=1, bboxes=None, page_size=None,
                  edge_geometry_on=False, attention="gat", attention_dropout=0.0, seed_base=0, training=True):
    """The reference's single GraphAttentionLayer (models.py:114) or the multi-head / stacked extension:
    every layer concatenates its heads (hidden_dim/n_heads channels each, written side by side), layers
    are chained; the last one writes the context columns comb[:, F:].
    ``edge_geometry_on``: the edge features of the batch (``bboxes``, ``page_size`` = (height, width)) are computed once
    and handed to every head.  ``attention``: the scoring mode of every head ('gat' | 'gatv2', gat_fwd).
    ``attention_dropout`` > 0: head (l, i) drops attention coefficients from its own stream
    attention_dropout_seed(``seed_base``, l, i) while it is in train mode (``training``: a bool or per-layer modes, the
    head's key is its prefix + ATTN_DROP_KEY); ``seed_base`` is the step's first decoder seed."""
    from .weights import check_attention_dropout, gat_prefixes
    prefixes = gat_prefixes(n_heads, n_gat_layers)
    attention_dropout = check_attention_dropout(attention_dropout)
    phi = None
    if edge_geometry_on:
        if bboxes is None or page_size is None:
            raise ValueError("edge_geometry needs the boxes and the page size (height, width)")
        phi = edge_geometry(bboxes, ctx, page_size)
    dh = D // n_heads
    layers, h, ldh, fin = [], comb, T, F
    for l, heads in enumerate(prefixes):
        last = l == len(prefixes) - 1
        out, ldo = (comb[:, F:], T) if last else (_empty((N, D), comb), D)
        drops = [(attention_dropout, attention_dropout_seed(seed_base, l, i))
                 if attention_dropout > 0 and is_train(training, p + ATTN_DROP_KEY) else None for i, p in enumerate(heads)]
        svs = [gat_fwd(h, ldh, N, fin, ctx, params, out[:, i * dh:], ldo, prefix=p, phi=phi, attention=attention,
                       drop=drops[i]) for i, p in enumerate(heads)]
        layers.append(dict(heads=svs, out=out))
        h, ldh, fin = out, ldo, D
    return layers


def gat_stack_bwd(layers, dcomb, T, N, F, D, params, gout=None):
    """dcomb[:, F:] = dL/d(context); accumulates dL/d(own features) into dcomb[:, :F]."""
    grads = {}
    g, ldg = dcomb[:, F:], T
    csr = gat_transpose(layers[0]["heads"][0]["ctx"])
    for l in reversed(range(len(layers))):
        heads = layers[l]["heads"]
        dh = D // len(heads)
        if l == 0:
            dst, ldd, acc0 = dcomb, T, True
        else:
            dst, ldd, acc0 = _empty((N, D), dcomb), D, False
        for i, sv in enumerate(heads):
            grads.update(gat_bwd(sv, g[:, i * dh:], ldg, params, dst, ldd, acc0 or i > 0, gout, csr))
        g, ldg = dst, ldd
    return grads


# ------------------------------------------------------------------------------- page readout
def page_start_of(bboxes, images, page_start=None, option="page_context_dim"):
    """The pages' row offsets (device int64 [B + 1]) without a host read: the batch's table when given, else from the
    page column of the page-sorted boxes and the page count of the images (HotPathTrainer._page_start's rule).
    ``option`` names the cfg entry that needs the table in the error of a batch that has neither."""
    if page_start is not None:
        return _check(page_start.contiguous(), torch.int64)
    if images is None:
        raise ValueError("%s: a batch without images must carry page_start (the pages' row offsets, "
                         "int64 [B + 1])" % option)
    pages = torch.arange(int(images.shape[0]) + 1, dtype=torch.float32, device=bboxes.device)
    return torch.searchsorted(bboxes[:, 0].contiguous(), pages)


def _linear_bwd(dy, ldy, x, ldx, W, N, n_out, n_in, db, dW, dx, lddx, accumulate):
    """Backward of y = x W^T (+ b) over N rows, W [n_out, n_in]: db = column sums of dy (cova_colsum; ``db`` None: no bias),
    dW = dy^T x, and dx = dy W written, or with ``accumulate`` added to what dx holds (cova_sgemm twice)."""
    if db is not None:
        call("cova_colsum", dy, ldy, N, n_out, db)
    call("cova_sgemm", 1, 0, n_out, n_in, N, dy, ldy, x, ldx, dW, n_in, None, 0)
    call("cova_sgemm", 0, 0, N, n_in, n_out, dy, ldy, W, n_in, dx, lddx, None, 1 if accumulate else 0)


def page_readout_fwd(h, ldh, N, F, page_start, params, out, ldo, prefix="page_readout."):
    """The page readout (cova_page_readout_fwd): P = h W^T by cova_sgemm, then per page the softmax of
    LeakyReLU(a . P_i + b) over its rows and r_p = sum beta_i P_i, written to the row out + n*ldo of every box of the page.
    h rows at h + n*ldh (F values); ``page_start`` device int64 [B + 1].  -> saved dict for page_readout_bwd."""
    _check(page_start, torch.int64)
    W = params[prefix + "W.weight"]
    aw, ab = params[prefix + "attention_layer.weight"], params[prefix + "attention_layer.bias"]
    G, B = W.shape[0], page_start.shape[0] - 1
    if W.shape[1] != F or aw.numel() != G:
        raise ValueError("%sW.weight %s / attention_layer.weight %s do not fit %d own features"
                         % (prefix, tuple(W.shape), tuple(aw.shape), F))
    P = _empty((N, G), h)
    call("cova_sgemm", 0, 1, N, G, F, h, ldh, W, F, P, G, None, 0)
    u, beta, r = _empty((N,), h), _empty((N,), h), _empty((B, G), h)
    call("cova_page_readout_fwd", P, G, aw, ab, page_start, B, N, G, LEAKY_SLOPE, u, beta, r, out, ldo)
    return dict(h=h, ldh=ldh, N=N, F=F, G=G, B=B, P=P, u=u, beta=beta, r=r, page_start=page_start, prefix=prefix)


def page_readout_bwd(sv, g, ldg, params, dh, lddh, gout=None):
    """g = dL/d(readout columns) (rows at g + n*ldg).  ACCUMULATES dL/dh into dh; returns the three parameter gradients."""
    N, F, G, B, prefix = sv["N"], sv["F"], sv["G"], sv["B"], sv["prefix"]
    W, aw = params[prefix + "W.weight"], params[prefix + "attention_layer.weight"]
    dP = _empty((N, G), g)
    daw = _gbuf(gout, prefix + "attention_layer.weight", (1, G), g)
    dab = _gbuf(gout, prefix + "attention_layer.bias", (1,), g)
    ws = _empty((query("cova_page_readout_workspace_floats", B, G),), g)
    call("cova_page_readout_bwd", g, ldg, sv["P"], G, sv["u"], sv["beta"], sv["r"], aw, sv["page_start"], B, N, G,
         LEAKY_SLOPE, dP, G, daw, dab, ws)
    dW = _gbuf(gout, prefix + "W.weight", (G, F), g)
    _linear_bwd(dP, G, sv["h"], sv["ldh"], W, N, G, F, None, dW, dh, lddh, True)
    return {prefix + "W.weight": dW, prefix + "attention_layer.weight": daw, prefix + "attention_layer.bias": dab}


# ------------------------------------------------------------------------------- page self-attention
# The attention core: what the stand-alone layer and every block of the page encoder share.  ``geo`` = (geometry.weight
# [heads, 8], bboxes, img_w, img_h) turns the box-geometry bias on (the _geo kernels), None leaves it off.
def _page_geometry(bboxes, N, page_size, what):
    """The inputs of the geometry bias -> (bboxes, img_w, img_h): ``bboxes`` dense float32 [N, 5] on the device and
    ``page_size`` = (height, width) in pixels.  ``what`` names the weight that needs them."""
    if bboxes is None or tuple(bboxes.shape) != (N, 5):
        raise ValueError("%s: the geometry bias needs bboxes [%d, 5]" % (what, N))
    _check(bboxes)
    img_h, img_w = _page_hw(page_size)
    return bboxes, img_w, img_h


# ``drop`` = (p, seed) with p in (0, 1) puts dropout on the probabilities (the _drop kernels), None leaves it off: four
# kernel pairs, picked by (geo, drop).
def _page_attn_core_fwd(qkv, ld, width, heads, page_start, geo, out, ldo, what="", drop=None):
    """cova_page_attn_fwd(_geo)(_drop) on the rows [Q | K | V] at qkv + n*ld -> lse [N, heads]; the output rows go to
    out + n*ldo (``width`` columns).  Rows outside every page are written by neither kernel."""
    N, B = qkv.shape[0], page_start.shape[0] - 1
    lse = _empty((N, heads), qkv)
    drop = check_page_drop(drop)                       # (a hand-made (p, seed) is held to the rule here, as gat_fwd's is)
    tail = () if drop is None else drop
    if geo is None:
        call("cova_page_attn_fwd_drop" if tail else "cova_page_attn_fwd", qkv, ld, page_start, B, N, width, heads, out, ldo,
             lse, *tail)
        return lse
    gw, bboxes, img_w, img_h = geo
    if tuple(gw.shape) != (heads, 8):
        raise ValueError("%sgeometry.weight %s does not fit %d heads" % (what, tuple(gw.shape), heads))
    call("cova_page_attn_fwd_geo_drop" if tail else "cova_page_attn_fwd_geo", qkv, ld, page_start, bboxes, gw, img_w, img_h,
         B, N, width, heads, out, ldo, lse, *tail)
    return lse


def _page_attn_core_bwd(g, ldg, qkv, ld, out, ldo, lse, width, heads, page_start, geo, dgeo, drop=None):
    """cova_page_attn_bwd(_geo)(_drop) -> dqkv [N, 3 width]; with ``geo`` the geometry weight's gradient goes to ``dgeo``
    (the kernel's workspace comes from the allocator); ``drop`` is the forward's.  dqkv is allocated here, as ZEROS: the
    kernels write the rows inside pages only, and both callers run GEMMs over all N rows of it."""
    N, B = qkv.shape[0], page_start.shape[0] - 1
    dqkv = torch.zeros((N, 3 * width), dtype=torch.float32, device=g.device)
    tail = () if drop is None else (float(drop[0]), int(drop[1]))
    if geo is None:
        call("cova_page_attn_bwd_drop" if tail else "cova_page_attn_bwd", g, ldg, qkv, ld, out, ldo, lse, page_start, B, N,
             width, heads, dqkv, 3 * width, *tail)
        return dqkv
    gw, bboxes, img_w, img_h = geo
    ws = _empty((query("cova_page_attn_geo_workspace_floats", B, N, heads),), g)
    call("cova_page_attn_bwd_geo_drop" if tail else "cova_page_attn_bwd_geo", g, ldg, qkv, ld, out, ldo, lse, page_start,
         bboxes, gw, img_w, img_h, B, N, width, heads, dqkv, 3 * width, dgeo, ws, *tail)
    return dqkv


def _page_drop_rate(dropout, option, training, key):
    """The rate a page layer drops at in this call: the checked ``dropout`` while its Dropout ``key`` is in train mode
    (is_train), else 0.0 (the plain launches)."""
    from .weights import check_page_dropout
    p = check_page_dropout(dropout, option)
    return p if p > 0.0 and is_train(training, key) else 0.0


def page_attn_fwd(h, ldh, N, F, page_start, params, heads, out, ldo, prefix="page_attention.", bboxes=None,
                  page_size=None, dropout=0.0, seed_base=0, training=True):
    """The page self-attention (cova_page_attn_fwd): [Q | K | V] = h qkv.weight^T by cova_sgemm, then per page and head the
    softmax of Q_i . K_j / sqrt(dh) over ALL rows j of the page and O_i = sum_j A_ij V_j, written to the rows out + n*ldo
    (E columns).  h rows at h + n*ldh (F values); ``page_start`` device int64 [B + 1].  -> saved dict for page_attn_bwd
    (qkv, lse [N, heads] and the output's place: the probabilities are recomputed).
    With ``geometry.weight`` [heads, 8] among the parameters the scores carry the box-geometry bias
    (cova_page_attn_fwd_geo): ``bboxes`` [N, 5] and ``page_size`` = (height, width) in pixels are then required.
    ``dropout`` > 0 (``page_attention_dropout``): while the layer's Dropout is in train mode (``training``: a bool
    or per-layer modes, key PAGE_ATTN_DROP_KEY) the probabilities are dropped from the stream
    page_dropout_seed(``seed_base``, weights.PAGE_ENCODER_MAX_LAYERS, 0) (cova_page_attn_fwd_drop / _geo_drop; ``seed_base``
    is the step's first decoder seed); the saved dict carries (p, seed) as ``drop`` for page_attn_bwd.  With 0, or in eval
    mode, exactly the calls above are issued."""
    from .weights import PAGE_ATTENTION_DROPOUT_OPTION, PAGE_ENCODER_MAX_LAYERS
    _check(page_start, torch.int64)
    p_drop = _page_drop_rate(dropout, PAGE_ATTENTION_DROPOUT_OPTION, training, PAGE_ATTN_DROP_KEY)
    drop = (p_drop, page_dropout_seed(seed_base, PAGE_ENCODER_MAX_LAYERS, 0)) if p_drop > 0.0 else None
    W = params[prefix + "qkv.weight"]
    E, B = W.shape[0] // 3, page_start.shape[0] - 1
    if W.shape[1] != F or W.shape[0] != 3 * E or E < 1:
        raise ValueError("%sqkv.weight %s does not fit %d own features" % (prefix, tuple(W.shape), F))
    gw = params.get(prefix + "geometry.weight")
    geo = None if gw is None else (gw,) + _page_geometry(bboxes, N, page_size, prefix + "geometry.weight")
    qkv = _empty((N, 3 * E), h)
    call("cova_sgemm", 0, 1, N, 3 * E, F, h, ldh, W, F, qkv, 3 * E, None, 0)
    lse = _page_attn_core_fwd(qkv, 3 * E, E, heads, page_start, geo, out, ldo, prefix, drop)
    sv = dict(h=h, ldh=ldh, N=N, F=F, E=E, B=B, heads=heads, qkv=qkv, lse=lse, out=out, ldo=ldo, page_start=page_start,
              prefix=prefix, drop=drop)
    if geo is not None:
        sv.update(bboxes=bboxes, img_w=geo[2], img_h=geo[3])
    return sv


def _saved_geo(sv, gw):
    """The core's ``geo`` of a backward, from what the forward saved (``bboxes`` there: it took the geometry bias)."""
    return (gw, sv["bboxes"], sv["img_w"], sv["img_h"]) if "bboxes" in sv else None


def page_attn_bwd(sv, g, ldg, params, dh, lddh, gout=None):
    """g = dL/d(attention columns) (rows at g + n*ldg).  ACCUMULATES dL/dh into dh; returns the weight gradient (and
    the geometry weight's, where the forward took the bias)."""
    N, F, E, prefix = sv["N"], sv["F"], sv["E"], sv["prefix"]
    grads = {}
    geo = _saved_geo(sv, params.get(prefix + "geometry.weight"))
    if geo is not None:
        grads[prefix + "geometry.weight"] = _gbuf(gout, prefix + "geometry.weight", (sv["heads"], 8), g)
    dqkv = _page_attn_core_bwd(g, ldg, sv["qkv"], 3 * E, sv["out"], sv["ldo"], sv["lse"], E, sv["heads"], sv["page_start"],
                               geo, grads.get(prefix + "geometry.weight"), sv.get("drop"))
    grads[prefix + "qkv.weight"] = dW = _gbuf(gout, prefix + "qkv.weight", (3 * E, F), g)
    _linear_bwd(dqkv, 3 * E, sv["h"], sv["ldh"], params[prefix + "qkv.weight"], N, 3 * E, F, None, dW, dh, lddh, True)
    return grads


# ------------------------------------------------------------------------------- page encoder
LN_EPS = 1e-5                         # nn.LayerNorm's default (weights.PAGE_ENCODER_EPS)


def layernorm_fwd(x, ldx, N, C, weight, bias, out, ldo):
    """cova_layernorm_fwd over the rows x + n*ldx -> (mean [N], rstd [N]); ``out`` rows at out + n*ldo."""
    mean, rstd = _empty((N,), x), _empty((N,), x)
    call("cova_layernorm_fwd", x, ldx, N, C, weight, bias, LN_EPS, out, ldo, mean, rstd)
    return mean, rstd


def layernorm_bwd(g, ldg, x, ldx, mean, rstd, weight, N, C, res, dx, lddx, dweight, dbias):
    """cova_layernorm_bwd: dx = (res or 0) + dL/dx (``res`` may be ``dx``: the stream gradient updated in place), dweight
    and dbias written; the workspace comes from the allocator."""
    ws = _empty((query("cova_layernorm_workspace_floats", N, C),), g)
    call("cova_layernorm_bwd", g, ldg, x, ldx, mean, rstd, weight, N, C, res, lddx if res is not None else 0, dx, lddx,
         dweight, dbias, ws)


def page_encoder_fwd(h, ldh, N, F, page_start, params, heads, layers, out, ldo, prefix="page_encoder.", bboxes=None,
                     page_size=None, dropout=0.0, seed_base=0, training=True):
    """The page encoder: x = h input.weight^T, then ``layers`` pre-LN transformer blocks restricted to pages,
        a = LN1(x); qkv = a qkv.weight^T; O = page attention of qkv; x += O out.weight^T + out.bias
        m = LN2(x); z = m ffn1.weight^T + ffn1.bias; f = GELU(z); x += f ffn2.weight^T + ffn2.bias
    and the final LN, written to the rows out + n*ldo (P columns).  The GEMMs are cova_sgemm (a residual add is its bias +
    accumulate form into a copy of the stream), the attention is cova_page_attn_fwd on the layer's qkv, or with
    ``geometry.weight`` [heads, 8] among a layer's parameters cova_page_attn_fwd_geo (``bboxes`` [N, 5] and ``page_size`` =
    (height, width) are then required); LayerNorm and GELU are cova_layernorm_fwd / cova_gelu_fwd.  attention_dropout and
    edge_geometry belong to the GAT and do not reach the encoder.
    ``dropout`` = p > 0 (``page_encoder_dropout``; torch's ``dropout=`` of nn.TransformerEncoderLayer): while the
    encoder's Dropout is in train mode (``training``: a bool or per-layer modes, key PAGE_ENC_DROP_KEY) every block runs
        x += drop1(out(Attn_drop(qkv(LN1(x)))));   x += drop2(ffn2(drop_h(GELU(ffn1(LN2(x))))))
    with layer l's four sites on the streams page_dropout_seed(``seed_base``, l, 0..3) (``seed_base``: the step's first
    decoder seed): the attention runs the _drop kernels, GELU is cova_gelu_fwd_drop, and each sublayer GEMM writes its
    output ``y`` (bias form) for cova_dropout_add_fwd, which stands in for the copy + accumulate pair.  No mask is stored;
    the saved dict carries ``drop`` = p and ``seed_base``.  With 0, or in eval mode, exactly the calls above are issued.
    h rows at h + n*ldh (F values); ``page_start`` device int64 [B + 1].  -> saved dict for page_encoder_bwd: per layer the
    stream ``x`` at both LayerNorm inputs with their ``mean`` / ``rstd`` and outputs, ``qkv``, ``lse``, ``O``, ``z``, ``f``."""
    from .weights import PAGE_ENCODER_DROPOUT_OPTION
    _check(page_start, torch.int64)
    p_drop = _page_drop_rate(dropout, PAGE_ENCODER_DROPOUT_OPTION, training, PAGE_ENC_DROP_KEY)
    seeds = (lambda l: tuple(page_dropout_seed(seed_base, l, i) for i in range(PAGE_DROP_SITES))) if p_drop > 0.0 else None
    W_in = params[prefix + "input.weight"]
    P, B = W_in.shape[0], page_start.shape[0] - 1
    if W_in.shape[1] != F or P < 1:
        raise ValueError("%sinput.weight %s does not fit %d own features" % (prefix, tuple(W_in.shape), F))
    geo_args = None
    if (prefix + "layers.0.geometry.weight") in params:
        geo_args = _page_geometry(bboxes, N, page_size, prefix + "layers.*.geometry.weight")
    x = _empty((N, P), h)
    call("cova_sgemm", 0, 1, N, P, F, h, ldh, W_in, F, x, P, None, 0)
    blocks = []
    for l in range(layers):
        p = "%slayers.%d." % (prefix, l)
        Wqkv, W1 = params[p + "qkv.weight"], params[p + "ffn1.weight"]
        M = W1.shape[0]
        if tuple(Wqkv.shape) != (3 * P, P) or W1.shape[1] != P or tuple(params[p + "ffn2.weight"].shape) != (P, M):
            raise ValueError("%s*: the layer's weights do not fit page_encoder_dim=%d" % (p, P))
        b = dict(prefix=p, M=M, x1=x)
        b["a"] = a = _empty((N, P), h)
        b["mean1"], b["rstd1"] = layernorm_fwd(x, P, N, P, params[p + "norm1.weight"], params[p + "norm1.bias"], a, P)
        b["qkv"] = qkv = _empty((N, 3 * P), h)
        call("cova_sgemm", 0, 1, N, 3 * P, P, a, P, Wqkv, P, qkv, 3 * P, None, 0)
        # rows outside every page are written by no attention kernel: they stay zero
        b["O"] = O = torch.zeros((N, P), dtype=torch.float32, device=h.device)
        geo = None if geo_args is None else (params[p + "geometry.weight"],) + geo_args
        sd = seeds(l) if seeds is not None else None
        b["lse"] = _page_attn_core_fwd(qkv, 3 * P, P, heads, page_start, geo, O, P, p,
                                       (p_drop, sd[0]) if sd is not None else None)
        x2 = _empty((N, P), h)
        if sd is None:
            x2.copy_(x)                               # (a device copy: the stream at LN1's input is kept for its backward)
            call("cova_sgemm", 0, 1, N, P, P, O, P, params[p + "out.weight"], P, x2, P, params[p + "out.bias"], 1)
        else:
            y = _empty((N, P), h)
            call("cova_sgemm", 0, 1, N, P, P, O, P, params[p + "out.weight"], P, y, P, params[p + "out.bias"], 0)
            call("cova_dropout_add_fwd", y, P, x, P, x2, P, N, P, p_drop, sd[1])
        b["x2"] = x2
        b["m"] = m = _empty((N, P), h)
        b["mean2"], b["rstd2"] = layernorm_fwd(x2, P, N, P, params[p + "norm2.weight"], params[p + "norm2.bias"], m, P)
        b["z"] = z = _empty((N, M), h)
        call("cova_sgemm", 0, 1, N, M, P, m, P, W1, P, z, M, params[p + "ffn1.bias"], 0)
        b["f"] = f = _empty((N, M), h)
        x = _empty((N, P), h)
        if sd is None:
            call("cova_gelu_fwd", z, M, N, M, f, M)
            x.copy_(x2)
            call("cova_sgemm", 0, 1, N, P, M, f, M, params[p + "ffn2.weight"], M, x, P, params[p + "ffn2.bias"], 1)
        else:
            call("cova_gelu_fwd_drop", z, M, N, M, f, M, p_drop, sd[2])        # f: the dropped activations, ffn2's input
            y = _empty((N, P), h)
            call("cova_sgemm", 0, 1, N, P, M, f, M, params[p + "ffn2.weight"], M, y, P, params[p + "ffn2.bias"], 0)
            call("cova_dropout_add_fwd", y, P, x2, P, x, P, N, P, p_drop, sd[3])
        blocks.append(b)
    mean, rstd = layernorm_fwd(x, P, N, P, params[prefix + "norm.weight"], params[prefix + "norm.bias"], out, ldo)
    sv = dict(h=h, ldh=ldh, N=N, F=F, P=P, B=B, heads=heads, layers=layers, blocks=blocks, x=x, mean=mean, rstd=rstd,
              page_start=page_start, prefix=prefix, drop=p_drop, seed_base=seed_base)
    if geo_args is not None:
        sv.update(bboxes=bboxes, img_w=geo_args[1], img_h=geo_args[2])
    return sv


def page_encoder_bwd(sv, g, ldg, params, dh, lddh, gout=None):
    """g = dL/d(encoder columns) (rows at g + n*ldg).  Walks the blocks backwards: per Linear _linear_bwd (cova_colsum for
    out.bias / ffn1.bias / ffn2.bias, the two cova_sgemm), cova_gelu_bwd, the attention core's backward and
    cova_layernorm_bwd with ``res`` = the stream gradient, which is so read and written once per LayerNorm.  Where the
    forward dropped (``drop`` > 0 in the saved dict) each sublayer's _linear_bwd is fed with cova_dropout_regen_bwd's
    output instead of the stream gradient, GELU's backward is cova_gelu_bwd_drop and the attention core takes the
    forward's (p, seed): every mask is regenerated from the forward's streams.  ACCUMULATES dL/dh into dh; returns every
    parameter gradient."""
    N, F, P, Hh, prefix = sv["N"], sv["F"], sv["P"], sv["heads"], sv["prefix"]
    p_drop = sv.get("drop", 0.0)
    grads = {}

    def buf(key, shape):
        grads[key] = t = _gbuf(gout, key, shape, g)
        return t

    gx = _empty((N, P), g)                 # the gradient on the residual stream
    layernorm_bwd(g, ldg, sv["x"], P, sv["mean"], sv["rstd"], params[prefix + "norm.weight"], N, P, None, gx, P,
                  buf(prefix + "norm.weight", (P,)), buf(prefix + "norm.bias", (P,)))
    gy = _empty((N, P), g) if p_drop > 0.0 else None        # a sublayer output's gradient: the stream's through its mask
    for l in reversed(range(len(sv["blocks"]))):
        b = sv["blocks"][l]
        p, M = b["prefix"], b["M"]
        sd = tuple(page_dropout_seed(sv["seed_base"], l, i) for i in range(PAGE_DROP_SITES)) if p_drop > 0.0 else None
        # x3 = x2 + f ffn2.weight^T + ffn2.bias
        df = _empty((N, M), g)
        if sd is not None:
            call("cova_dropout_regen_bwd", gx, P, gy, P, N, P, p_drop, sd[3])
        _linear_bwd(gy if sd is not None else gx, P, b["f"], M, params[p + "ffn2.weight"], N, P, M,
                    buf(p + "ffn2.bias", (P,)), buf(p + "ffn2.weight", (P, M)), df, M, False)
        dz = _empty((N, M), g)
        if sd is not None:
            call("cova_gelu_bwd_drop", df, M, b["z"], M, N, M, dz, M, p_drop, sd[2])
        else:
            call("cova_gelu_bwd", df, M, b["z"], M, N, M, dz, M)
        dm = _empty((N, P), g)
        _linear_bwd(dz, M, b["m"], P, params[p + "ffn1.weight"], N, M, P, buf(p + "ffn1.bias", (M,)),
                    buf(p + "ffn1.weight", (M, P)), dm, P, False)
        layernorm_bwd(dm, P, b["x2"], P, b["mean2"], b["rstd2"], params[p + "norm2.weight"], N, P, gx, gx, P,
                      buf(p + "norm2.weight", (P,)), buf(p + "norm2.bias", (P,)))
        # x2 = x1 + O out.weight^T + out.bias
        dO = dm                                # (dead by now: reuse)
        if sd is not None:
            call("cova_dropout_regen_bwd", gx, P, gy, P, N, P, p_drop, sd[1])
        _linear_bwd(gy if sd is not None else gx, P, b["O"], P, params[p + "out.weight"], N, P, P,
                    buf(p + "out.bias", (P,)), buf(p + "out.weight", (P, P)), dO, P, False)
        geo = _saved_geo(sv, params.get(p + "geometry.weight"))
        dqkv = _page_attn_core_bwd(dO, P, b["qkv"], 3 * P, b["O"], P, b["lse"], P, Hh, sv["page_start"], geo,
                                   buf(p + "geometry.weight", (Hh, 8)) if geo is not None else None,
                                   (p_drop, sd[0]) if sd is not None else None)
        da = _empty((N, P), g)
        _linear_bwd(dqkv, 3 * P, b["a"], P, params[p + "qkv.weight"], N, 3 * P, P, None, buf(p + "qkv.weight", (3 * P, P)),
                    da, P, False)
        layernorm_bwd(da, P, b["x1"], P, b["mean1"], b["rstd1"], params[p + "norm1.weight"], N, P, gx, gx, P,
                      buf(p + "norm1.weight", (P,)), buf(p + "norm1.bias", (P,)))
    _linear_bwd(gx, P, sv["h"], sv["ldh"], params[prefix + "input.weight"], N, P, F, None,
                buf(prefix + "input.weight", (P, F)), dh, lddh, True)
    return grads


# ------------------------------------------------------------------------------- decoder
def dropout_fwd(x, ld, N, C, p, seed, mask=None):
    out = _empty((N, C), x)
    given = mask is not None
    if not given:
        mask = _empty((N, C), x, torch.uint8)
    else:
        _check(mask, torch.uint8)
    call("cova_dropout_fwd", x, ld, out, C, mask, N, C, float(p), int(seed), 1 if given else 0)
    return out, mask


def decoder_fwd(x, N, T, params, buffers, training, p, seeds=(0, 0), masks=None):
    """models.py:83-90 on the concatenated features x [N,T]: Dropout, Linear, BN1d, ReLU, Dropout,
    Linear.  ``masks`` (two uint8 [N,T] keep-masks) override the generated ones (parity tests).  Each Dropout
    ("decoder.0", "decoder.3") and the BatchNorm follow their own mode in ``training`` (is_train)."""
    NC = params["decoder.5.weight"].shape[0]
    active = p > 0 or masks is not None
    drop1 = is_train(training, DROPOUT_KEYS[0]) and active
    drop = is_train(training, DROPOUT_KEYS[1]) and active
    sv = dict(N=N, T=T, NC=NC, drop=drop, drop1=drop1, p=p)
    xd, m1 = dropout_fwd(x, T, N, T, p, seeds[0], masks[0] if masks else None) if drop1 else (x, None)
    z = _empty((N, T), x)
    call("cova_sgemm", 0, 1, N, T, T, xd, T, params["decoder.1.weight"], T, z, T,
         params["decoder.1.bias"], 0)
    y = _empty((N, T), x)
    if drop:
        st, yd, m2 = bn1d_fwd(z, T, N, T, "decoder.2.", params, buffers, training, y, T, True,
                              drop=(p, seeds[1], masks[1] if masks else None))
    else:
        st, yd, m2 = bn1d_fwd(z, T, N, T, "decoder.2.", params, buffers, training, y, T, True), y, None
    logits = _empty((N, NC), x)
    call("cova_linear_small_fwd", yd, T, params["decoder.5.weight"], params["decoder.5.bias"], logits,
         N, T, NC)
    sv.update(xd=xd, m1=m1, z=z, y=y, st=st, yd=yd, m2=m2)
    return logits, sv


def decoder_bwd(sv, dlogits, params, gout=None):
    """-> (dL/dx [N,T], param grads)."""
    N, T, NC, p = sv["N"], sv["T"], sv["NC"], sv["p"]
    _check(dlogits)
    dyd = _empty((N, T), dlogits)
    dW2 = _gbuf(gout, "decoder.5.weight", (NC, T), dlogits)
    db2 = _gbuf(gout, "decoder.5.bias", (NC,), dlogits)
    call("cova_linear_small_bwd", dlogits, sv["yd"], T, params["decoder.5.weight"], dyd, T, dW2, db2,
         N, T, NC)
    dz = _empty((N, T), dlogits)
    db1 = _gbuf(gout, "decoder.1.bias", (T,), dlogits)
    dg, db = bn_backward(dyd, T, sv["y"], T, sv["z"], T, sv["st"], N, dz, T, None, 0, gout, "decoder.2.",
                         drop=(sv["m2"], p) if sv["drop"] else None, colsum=db1)
    dW1 = _gbuf(gout, "decoder.1.weight", (T, T), dlogits)
    call("cova_sgemm", 1, 0, T, T, N, dz, T, sv["xd"], T, dW1, T, None, 0)
    dx = dyd        # (dead by now: reuse)
    if sv.get("drop1", sv["drop"]):  # the first Dropout's backward in the GEMM's epilogue (one launch less, same bits)
        call("cova_sgemm_dropout_bwd", 0, 0, N, T, T, dz, T, params["decoder.1.weight"], T, dx, T, sv["m1"], float(p))
    else:
        call("cova_sgemm", 0, 0, N, T, T, dz, T, params["decoder.1.weight"], T, dx, T, None, 0)
    grads = {"decoder.1.weight": dW1, "decoder.1.bias": db1, "decoder.2.weight": dg,
             "decoder.2.bias": db, "decoder.5.weight": dW2, "decoder.5.bias": db2}
    return dx, grads


# ------------------------------------------------------------------------------- whole model
@on_device_of(3)
def model_fwd(cfg, params, buffers, images, bboxes, additional_feats, context_indices, training,
              seeds=(0, 0), masks=None, save=True, plan=None, visual_feats=None, page_size=None, page_start=None):
    """CoVA.forward (models.py:94-122) -> (logits [N,n_classes], saved-for-backward or None).
    ``page_start`` (device int64 [B + 1], the pages' row offsets) is read by the context layers that work per page
    (weights.CONTEXT_LAYERS: cfg["page_context_dim"], cfg["page_attention_dim"], cfg["page_encoder_dim"]) only: the batch's
    table when given, else derived on the device from the page column of ``bboxes`` and the page count of ``images``
    (page_start_of); a batch without either raises ValueError.
    ``page_size`` = (height, width) of the pages, read by the geometry options (_geometry_on) only: by default
    ``images.shape[2:]``; a batch without images (``visual_feats``) must name it (DeviceDataset batches carry it) or
    cfg["page_size"] must.
    ``training``: a bool (whole model) or per-layer modes {BatchNorm prefix / Dropout name: bool} (is_train).
    ``plan`` (grad_plan, with ``save``): without its "convstack" stage the conv stack keeps no activations.
    ``visual_feats`` = (table [R, n_vis], row_ids int32 [N]) (features.FeatureCache): the conv stack and the RoI op are
    skipped and cova_feat_rows_gather fills comb[:, :n_vis]; ``images`` may be None; with ``save`` the plan must lack
    "convstack" (nothing is kept to run that backward from)."""
    if visual_feats is not None:
        return _model_fwd_cached(cfg, params, buffers, bboxes, additional_feats, context_indices, training, seeds, masks,
                                 save, plan, visual_feats, page_size, page_start)
    PH, PW = cfg["roi_output_size"]
    n_vis = (C256 if is_bottleneck(params) else C128 if has_layer2(params) else C64) * PH * PW
    sv = _head_saved(cfg, n_vis, bboxes, images, page_size or cfg.get("page_size") or tuple(images.shape[2:]), page_start)
    N, T = sv["N"], sv["T"]
    align = cfg.get("roi_op", "pool") == "align"
    save_conv = save and (plan is None or "convstack" in plan)
    feat, sv["conv"] = convstack_fwd(images, params, buffers, training, save_conv, lazy_out=not align)
    sv["comb"] = comb = _empty((N, T), images)
    scale = cfg.get("spatial_scale") or feat.shape[1] / images.shape[2]   # models.py:56
    if align:
        sv["roi"] = roialign_fwd(feat, bboxes, (PH, PW), scale, cfg.get("sampling_ratio", 2),
                                 cfg.get("roi_aligned", False), comb, T)
    else:
        sv["roi"] = roipool_fwd(feat, bboxes, (PH, PW), scale, comb, T)
    return _head_fwd(cfg, params, buffers, bboxes, additional_feats, context_indices, training, seeds, masks, save, sv)


def _head_saved(cfg, n_vis, bboxes, images, page_size, page_start):
    """The saved dict both forms of model_fwd start from: the head's layout (weights.head_layout) as N, F, T, n_vis, Hd, A
    and one width per context layer (D, G, E, P), the page size, and the page table where a layer that is on reads one."""
    layout = head_layout(cfg, n_vis)
    if layout.page_option is not None:
        page_start = page_start_of(bboxes, images, page_start, layout.page_option)
    sv = dict(cfg=cfg, N=bboxes.shape[0], F=layout.F, T=layout.T, n_vis=n_vis, Hd=layout.Hd, A=layout.A, layout=layout,
              page_size=page_size, page_start=page_start)
    for layer, (_, _, width) in zip(CONTEXT_LAYERS, layout.layers):
        sv[layer.letter] = width
    return sv


def _geometry_on(cfg, sv, params, option, key=None):
    """A geometry option of ``cfg`` -> bool.  On, it needs the page size (a batch without images must carry it); and the
    parameters must agree with it: ``key``, the weight it adds, is there exactly when it is on."""
    on = bool(cfg.get(option, False))
    if on and sv.get("page_size") is None:
        raise ValueError("%s: a batch without images must carry page_size = (height, width) (or the configuration a "
                         "'page_size')" % option)
    if key is not None and on != (key in params):
        raise ValueError("%s=%r, but the parameters %s %s" % (option, on, "lack" if on else "hold", key))
    return on


# Per context layer its forward and backward behind one signature each.  The forward writes the columns ``out`` (rows at
# out + n*T) and returns what its backward needs; the backward reads g = dL/d(those columns) and ACCUMULATES dL/d(own
# features) into dcomb[:, :F].  Both walks below follow weights.CONTEXT_LAYERS, where the order is stated.
def _gat_ctx_fwd(cfg, params, sv, out, bboxes, ctx, training, seeds):
    edge = _geometry_on(cfg, sv, params, "edge_geometry")       # (gat_fwd holds every head's edge_layer.weight to it)
    return gat_stack_fwd(sv["comb"], sv["T"], sv["N"], sv["F"], sv["D"], ctx, params, cfg.get("n_heads", 1),
                         cfg.get("n_gat_layers", 1), bboxes if edge else None, sv.get("page_size"), edge,
                         cfg.get("attention", "gat"), cfg.get("attention_dropout", 0.0), seeds[0], training)


def _gat_ctx_bwd(sv, g, dcomb, params, gout):
    return gat_stack_bwd(sv["gat"], dcomb, sv["T"], sv["N"], sv["F"], sv["D"], params, gout)


def _readout_ctx_fwd(cfg, params, sv, out, bboxes, ctx, training, seeds):
    return page_readout_fwd(sv["comb"], sv["T"], sv["N"], sv["F"], sv["page_start"], params, out, sv["T"])


def _page_attn_ctx_fwd(cfg, params, sv, out, bboxes, ctx, training, seeds):
    geo = _geometry_on(cfg, sv, params, "page_attention_geometry", "page_attention.geometry.weight")
    return page_attn_fwd(sv["comb"], sv["T"], sv["N"], sv["F"], sv["page_start"], params, cfg.get("page_attention_heads", 1),
                         out, sv["T"], bboxes=bboxes if geo else None, page_size=sv.get("page_size"),
                         dropout=cfg.get("page_attention_dropout", 0.0), seed_base=seeds[0], training=training)


def _page_enc_ctx_fwd(cfg, params, sv, out, bboxes, ctx, training, seeds):
    geo = _geometry_on(cfg, sv, params, "page_encoder_geometry", "page_encoder.layers.0.geometry.weight")
    return page_encoder_fwd(sv["comb"], sv["T"], sv["N"], sv["F"], sv["page_start"], params,
                            cfg.get("page_encoder_heads", 1), cfg.get("page_encoder_layers", 1), out, sv["T"],
                            bboxes=bboxes if geo else None, page_size=sv.get("page_size"),
                            dropout=cfg.get("page_encoder_dropout", 0.0), seed_base=seeds[0], training=training)


def _page_ctx_bwd(key, bwd):
    return lambda sv, g, dcomb, params, gout: bwd(sv[key], g, sv["T"], params, dcomb, sv["T"], gout)


CONTEXT_STAGES = {"gat": (_gat_ctx_fwd, _gat_ctx_bwd),
                  "readout": (_readout_ctx_fwd, _page_ctx_bwd("readout", page_readout_bwd)),
                  "page_attn": (_page_attn_ctx_fwd, _page_ctx_bwd("page_attn", page_attn_bwd)),
                  "page_enc": (_page_enc_ctx_fwd, _page_ctx_bwd("page_enc", page_encoder_bwd))}
assert tuple(CONTEXT_STAGES) == tuple(layer.key for layer in CONTEXT_LAYERS)


def _head_fwd(cfg, params, buffers, bboxes, additional_feats, context_indices, training, seeds, masks, save, sv):
    """Everything behind the visual columns of ``sv["comb"]``: positional encoder, additional features, the context
    layers that are on, decoder."""
    N, T, n_vis, Hd, A, comb = (sv[k] for k in ("N", "T", "n_vis", "Hd", "A", "comb"))
    if Hd > 0:
        sv["bbox"] = bbox_fwd(bboxes, params, buffers, training, comb[:, n_vis:], T)
    if A > 0:
        _check(additional_feats)
        sv["addl_in"] = additional_feats
        sv["addl"] = bn1d_fwd(additional_feats, A, N, A, "bn_additional_feat.", params, buffers,
                              training, comb[:, n_vis + Hd:], T, False)
    for key, offset, width in sv["layout"].layers:
        if width > 0:
            sv[key] = CONTEXT_STAGES[key][0](cfg, params, sv, comb[:, offset:], bboxes, context_indices, training, seeds)
    logits, sv["dec"] = decoder_fwd(comb, N, T, params, buffers, training, cfg["drop_prob"], seeds,
                                    masks)
    return logits, (sv if save else None)


def check_visual_feats(cfg, visual_feats, N):
    """Host-side contract of (table, row_ids): a dense f32 table [R, n_vis] and one int32 row id per box, on one device.
    Id VALUES are not read (a device sync); cova_feat_rows_gather writes zeros for an id outside [0, R)."""
    try:
        table, row_ids = visual_feats
    except (TypeError, ValueError):
        raise ValueError("visual_feats must be (table [R, n_vis], row_ids int32 [N])")
    n_vis = backbone_feat(cfg)
    if not (torch.is_tensor(table) and table.dim() == 2 and table.shape[1] == n_vis and table.dtype == torch.float32
            and table.is_contiguous()):
        raise ValueError("visual_feats: the table must be a dense float32 [R, %d] tensor (n_vis of this configuration), "
                         "got %s" % (n_vis, (tuple(table.shape), table.dtype) if torch.is_tensor(table) else type(table)))
    if not (torch.is_tensor(row_ids) and row_ids.dim() == 1 and row_ids.dtype == torch.int32 and row_ids.is_contiguous()):
        raise ValueError("visual_feats: row_ids must be a contiguous int32 vector")
    if row_ids.shape[0] != N:
        raise ValueError("visual_feats: %d row ids for %d boxes" % (row_ids.shape[0], N))
    if table.shape[0] == 0 and N > 0:
        raise ValueError("visual_feats: %d boxes and an empty table" % N)
    if row_ids.device != table.device:
        raise ValueError("visual_feats: table on %s, row_ids on %s" % (table.device, row_ids.device))
    return table, row_ids


@on_device_of(3)
def _model_fwd_cached(cfg, params, buffers, bboxes, additional_feats, context_indices, training, seeds, masks, save, plan,
                      visual_feats, page_size=None, page_start=None):
    """model_fwd with the visual columns taken from a feature table: no conv stack, no RoI op."""
    N = bboxes.shape[0]
    table, row_ids = check_visual_feats(cfg, visual_feats, N)
    if save and (plan is None or "convstack" in plan):
        raise ValueError("model_fwd: cached visual features keep nothing for the conv-stack backward; the gradient plan "
                         "must leave out 'convstack' (a frozen conv stack)")
    n_vis = table.shape[1]
    sv = _head_saved(cfg, n_vis, bboxes, None, page_size or cfg.get("page_size"), page_start)
    T = sv["T"]
    sv["conv"] = sv["roi"] = None
    sv["comb"] = comb = _empty((N, T), bboxes)
    call("cova_feat_rows_gather", table, table.shape[0], n_vis, row_ids, N, comb, T)
    return _head_fwd(cfg, params, buffers, bboxes, additional_feats, context_indices, training, seeds, masks, save, sv)


@on_device_of(1)
def model_bwd(sv, dlogits, params, gout=None, after_head=None, want_dimg=False, plan=None):
    """-> {state_dict key: gradient} for every trainable parameter (+ "__images__" with ``want_dimg``).  ``gout`` (optional)
    maps keys to pre-allocated destinations, e.g. views into one flat all-reduce bucket.
    ``after_head`` (optional callable) runs once every gradient outside the conv stack is final
    (the trainer starts their all-reduce there, under the conv-stack backward).
    ``plan`` (grad_plan; None = every gradient): the backward stages it leaves out are not launched and their gradients
    are absent from the result (the forward must have had the same plan)."""
    if plan is not None and want_dimg:
        plan = plan | {"convstack", "stem", "layer1"}
    N, T, n_vis, Hd, A = (sv[k] for k in ("N", "T", "n_vis", "Hd", "A"))
    dcomb, grads = decoder_bwd(sv["dec"], dlogits, params, gout)
    for key, offset, width in sv["layout"].layers:          # (the forward's order: weights.CONTEXT_LAYERS says why)
        if width > 0:
            grads.update(CONTEXT_STAGES[key][1](sv, dcomb[:, offset:], dcomb, params, gout))
    if A > 0 and (plan is None or "addl" in plan):
        st = sv["addl"]
        dz = _empty((N, A), dcomb)
        dg, db = bn_backward(dcomb[:, n_vis + Hd:], T, None, 0, sv["addl_in"], A, st, N, dz, A, None, 0,
                             gout, "bn_additional_feat.")
        grads["bn_additional_feat.weight"], grads["bn_additional_feat.bias"] = dg, db
    if Hd > 0 and (plan is None or "bbox" in plan):
        grads.update(bbox_bwd(sv["bbox"], dcomb[:, n_vis:], T, gout))
    if after_head is not None:
        after_head()
    conv = sv["conv"]
    if plan is not None and "convstack" not in plan:
        return grads
    if conv is None:
        raise RuntimeError("model_bwd: the forward kept no conv-stack activations (its plan had no 'convstack' stage)")
    if N > 0 and sv["roi"]["zmax"] is not None:
        dfeat, head_part = roipool_bwd_bn(sv["roi"], dcomb, T, conv["last"], gout)
        grads.update(convstack_bwd(conv, dfeat, gout, head_part, params, want_dimg, plan))
    else:
        dfeat = roialign_bwd(sv["roi"], dcomb, T) if sv["roi"].get("kind") == "align" else roipool_bwd(sv["roi"], dcomb, T)
        grads.update(convstack_bwd(conv, dfeat, gout, None, params, want_dimg, plan))
    return grads


def ce_sum(logits, labels, want_grad=True, gscale=1.0):
    """CrossEntropyLoss(reduction='sum') + argmax (main.py:139, train.py:53,56)."""
    N, NC = logits.shape
    loss = _empty((1,), logits)
    dl = _empty((N, NC), logits) if want_grad else None
    pred = _empty((N,), logits, torch.int64)
    call("cova_ce_sum", logits, labels, N, NC, float(gscale), loss, dl, pred)
    return loss, dl, pred


# ------------------------------------------------------------------------------------------- page decoding
DECODE_MODES = ("column", "joint")
DECODE_SCORES = ("logit", "map")                     # the score_mode of cova_page_joint_decode is the index
JOINT_MAX_CLASSES = 7


def check_decode(decode, score, n_classes, k=1):
    """Host validation of a page decoding mode (ValueError each) -> the score_mode of cova_page_joint_decode.
    "column": the arg-max of every class column on its own; "joint": one distinct box per class (k must be 1, at most
    7 classes: the kernel enumerates up to 7^6 assignments a page)."""
    if decode not in DECODE_MODES:
        raise ValueError("decode must be one of %s, got %r" % (DECODE_MODES, decode))
    if score not in DECODE_SCORES:
        raise ValueError("the decoding score must be one of %s, got %r" % (DECODE_SCORES, score))
    if decode == "joint":
        if int(k) != 1:
            raise ValueError("decode=\"joint\" decides one box per class: k must be 1, got %r" % (k,))
        if not 2 <= int(n_classes) <= JOINT_MAX_CLASSES:
            raise ValueError("decode=\"joint\" takes 2..%d classes, got %r" % (JOINT_MAX_CLASSES, n_classes))
    return DECODE_SCORES.index(score)


# ------------------------------------------------------------------------------------------- configurable criterion
LOSS_MAX_CLASSES = 16                               # = COVA_MAX_CLASSES (csrc/rows.h), the one class limit of the row and page kernels
LOSS_REDUCTIONS = ("sum", "mean")


def check_loss_options(n_classes, class_weight=None, label_smoothing=0.0, focal_gamma=0.0, ignore_index=None,
                       reduction="sum"):
    """Host validation of the criterion's options (ValueError each) -> normalised dict for ce_loss_fwd / ce_loss_bwd.
    ``class_weight``: anything torch.as_tensor takes, or None; it is only checked here, not stored."""
    import math
    if not 0 < int(n_classes) <= LOSS_MAX_CLASSES:
        raise ValueError("the criterion kernels take 1..%d classes, got %r" % (LOSS_MAX_CLASSES, n_classes))
    if reduction not in LOSS_REDUCTIONS:
        raise ValueError("loss reduction must be one of %s, got %r" % (LOSS_REDUCTIONS, reduction))
    eps, gamma = float(label_smoothing), float(focal_gamma)
    if not 0.0 <= eps < 1.0:
        raise ValueError("label_smoothing must be in [0, 1), got %r" % (label_smoothing,))
    if not (gamma == 0.0 or (gamma >= 1.0 and math.isfinite(gamma))):
        raise ValueError("focal_gamma must be 0 (cross-entropy) or a finite value >= 1, got %r" % (focal_gamma,))
    if gamma != 0.0 and eps != 0.0:
        raise ValueError("focal_gamma and label_smoothing cannot be combined")
    if ignore_index is not None:
        ignore_index = int(ignore_index)
        if 0 <= ignore_index < int(n_classes):
            raise ValueError("ignore_index %d names a class (n_classes = %d)" % (ignore_index, n_classes))
    if class_weight is not None:
        w = torch.as_tensor(class_weight).detach().double().cpu()
        if w.dim() != 1 or w.numel() != int(n_classes):
            raise ValueError("class_weight must hold n_classes = %d values, got shape %s" % (n_classes, tuple(w.shape)))
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError("class_weight must be finite and non-negative, got %s" % w.tolist())
    return dict(label_smoothing=eps, focal_gamma=gamma, ignore_index=ignore_index, reduction=reduction)


def _loss_args(opts):
    ig = opts.get("ignore_index")
    return (float(opts.get("label_smoothing", 0.0)), float(opts.get("focal_gamma", 0.0)), 0 if ig is None else int(ig),
            0 if ig is None else 1)


def ce_loss_fwd(logits, labels, class_weight, opts, metrics=None, want_pred=True, workspace=None):
    """Phase 1 of the configurable criterion -> (acc float64 [3] = numerator, denominator, kept rows; pred).  Adds the
    batch to the device counters ``metrics`` (int64 [NC*NC + 4]) when given.  No host read."""
    N, NC = logits.shape
    n_ws = query("cova_ce_loss_workspace_doubles", N)
    if workspace is None or workspace.numel() < n_ws:
        workspace = _empty((n_ws,), logits, torch.float64)
    acc = _empty((3,), logits, torch.float64)
    pred = _empty((N,), logits, torch.int64) if want_pred else None
    call("cova_ce_loss_fwd", logits, labels, N, NC, class_weight, *_loss_args(opts), acc, pred, metrics, workspace)
    return acc, pred


def ce_loss_bwd(logits, labels, class_weight, opts, acc, grad_scale=None, want_loss=True, want_grad=True):
    """Phase 2: ``acc`` (device; all-reduced first under data parallelism with "mean") -> (loss f32 [1], dlogits)."""
    N, NC = logits.shape
    loss = _empty((1,), logits) if want_loss else None
    dl = _empty((N, NC), logits) if want_grad else None
    call("cova_ce_loss_bwd", logits, labels, N, NC, class_weight, *_loss_args(opts), acc,
         1 if opts.get("reduction", "sum") == "mean" else 0, grad_scale, loss, dl)
    return loss, dl


# ------------------------------------------------------------------------------------------- hard-negative mining
MINED_OUT = -(1 << 63)      # drop label of a caller without an ignore label of its own: no class, no torch default


def check_mining_options(ratio, min_keep=0):
    """Host validation of the mining options (ValueError each) -> (ratio as float or None = off, min_keep as int)."""
    import math
    import numbers
    if ratio is not None:
        if isinstance(ratio, bool) or not isinstance(ratio, numbers.Real) or not math.isfinite(ratio) or ratio < 0:
            raise ValueError("hard_negative_ratio must be None (off) or a finite number >= 0, got %r" % (ratio,))
        ratio = float(ratio)
    if isinstance(min_keep, bool) or not isinstance(min_keep, numbers.Integral) or min_keep < 0:
        raise ValueError("hard_negative_min must be an integer >= 0, got %r" % (min_keep,))
    return ratio, int(min_keep)


def hard_negative_select(logits, labels, page_start, ratio, min_keep, drop_label, want_scores=False, want_counts=False):
    """cova_hard_negative_select: per page (``page_start`` device int64 [B+1]) keep the positives and the
    max(min_keep, floor(ratio * positives)) background rows with the highest lse - l[0]; the other background rows get
    ``drop_label`` -> (labels_out int64 [N], scores f32 [N] or None, counts int32 [B, 3] = positives, background, kept
    background, or None).  One launch, no host read."""
    ratio, min_keep = check_mining_options(ratio, min_keep)
    if ratio is None:
        raise ValueError("hard_negative_select needs a ratio (None means that mining is off)")
    N, NC = logits.shape
    B = page_start.shape[0] - 1
    if page_start.dim() != 1 or B < 1 or labels.shape != (N,):
        raise ValueError("hard_negative_select takes logits [N, C], labels [N] and page_start [B + 1], B >= 1; got %s, %s, %s"
                         % (tuple(logits.shape), tuple(labels.shape), tuple(page_start.shape)))
    _check(logits), _check(labels, torch.int64), _check(page_start, torch.int64)
    out = _empty((N,), logits, torch.int64)
    scores = _empty((N,), logits) if want_scores else None
    counts = _empty((B, 3), logits, torch.int32) if want_counts else None
    call("cova_hard_negative_select", logits, labels, page_start, B, N, NC, ratio, min_keep, int(drop_label), out, scores,
         counts)
    return out, scores, counts


# ------------------------------------------------------------------------------------------- per-page ranking loss
def check_rank_options(page_rank_weight):
    """Host validation of the ranking term's weight (ValueError) -> float; 0 means that the term is off."""
    import math
    import numbers
    w = page_rank_weight
    if isinstance(w, bool) or not isinstance(w, numbers.Real) or not math.isfinite(w) or w < 0:
        raise ValueError("page_rank_weight must be a finite number >= 0 (0: off), got %r" % (w,))
    return float(w)


def _rank_shapes(logits, labels, page_start):
    N, NC = logits.shape
    B = page_start.shape[0] - 1
    if page_start.dim() != 1 or B < 1 or labels.shape != (N,):
        raise ValueError("the page ranking loss takes logits [N, C], labels [N] and page_start [B + 1], B >= 1; got %s, %s, %s"
                         % (tuple(logits.shape), tuple(labels.shape), tuple(page_start.shape)))
    _check(logits), _check(labels, torch.int64), _check(page_start, torch.int64)
    return B, N, NC


def _rank_ignore(opts):
    ig = opts.get("ignore_index")
    return (0, 0) if ig is None else (int(ig), 1)


def page_rank_loss_fwd(logits, labels, page_start, class_weight, opts):
    """Phase 1 of the per-page ranking loss (cova_page_rank_loss_fwd): per page of ``page_start`` (device int64 [B + 1])
    and class c >= 1 the list of the page's candidate rows in column c -> (lists float64 [B, NC-1, 4] = lse of the
    candidates, lse of the targets, candidate count, target count; acc float64 [3] = sum w_c L_pc, sum w_c, scored
    lists).  ``opts`` gives the ignore label ("ignore_index", None: none).  Two launches, no host read."""
    B, N, NC = _rank_shapes(logits, labels, page_start)
    lists = _empty((B, max(NC - 1, 0), 4), logits, torch.float64)
    acc = _empty((3,), logits, torch.float64)
    call("cova_page_rank_loss_fwd", logits, labels, page_start, B, N, NC, class_weight, *_rank_ignore(opts), lists, acc)
    return lists, acc


def page_rank_loss_bwd(logits, labels, page_start, class_weight, opts, lists, acc, rank_weight, grad_scale=None,
                       want_loss=True, want_grad=True, into=None):
    """Phase 2: ``lists`` and ``acc`` (device; all-reduced first under data parallelism with "mean") -> (loss f32 [1] =
    rank_weight * R, dlogits).  ``into`` = (loss or None, dlogits or None): the term and its gradient are added to these
    tensors (the outputs of ce_loss_bwd on the same stream) instead, and they are returned."""
    B, N, NC = _rank_shapes(logits, labels, page_start)
    rank_weight = float(rank_weight)
    if into is None:
        loss = _empty((1,), logits) if want_loss else None
        dl = _empty((N, NC), logits) if want_grad else None
    else:
        loss, dl = into
        for t, shape in ((loss, (1,)), (dl, (N, NC))):
            if t is not None:
                _check(t)
                if tuple(t.shape) != shape:
                    raise ValueError("page_rank_loss_bwd: cannot accumulate into a tensor of shape %s, expected %s"
                                     % (tuple(t.shape), shape))
    call("cova_page_rank_loss_bwd", logits, labels, page_start, B, N, NC, class_weight, *_rank_ignore(opts), lists, acc,
         rank_weight, 1 if opts.get("reduction", "sum") == "mean" else 0, grad_scale, loss, dl, 0 if into is None else 1)
    return loss, dl
