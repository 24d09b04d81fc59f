"""Drop-in mirror of the reference's ``models.py``: ``CoVA`` and ``GraphAttentionLayer``.

Same constructor signature (reference models.py:10-21, called positionally with 9 arguments at
main.py:122-132 / evaluate.py:187-197), same ``forward`` contract (models.py:94-122), same public
members used by the reference's scripts (``n_classes``, ``class_names``, ``gat(...,
return_attn_wts)``, ``_get_visual_features``, ``_get_bbox_features``, ``bn_additional_feat``;
extract_attn_wts_and_visualize.py:117-124) and the same 50 ``state_dict`` keys, so reference
checkpoints load unchanged and ``train.py`` / ``evaluate.py`` can drive it as they drive the
original.

Everything on the device is executed by the hand-written HIP kernels behind
``include/cova_hip.h``; the ``nn.Conv2d`` / ``nn.BatchNorm*`` / ``nn.Linear`` objects below are
parameter containers only (they give the reference's parameter names and shapes) and their own
``forward`` is never used.  Inputs must live on a ROCm device; there is no CPU fallback.
"""
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import engine
from .weights import (EDGE_FEATURES, PAGE_ATTENTION_DROPOUT_OPTION, PAGE_ENCODER_DROPOUT_OPTION, PAGE_ENCODER_OPTIONS,
                      attention_of, backbone_channels, check_attention, check_attention_dropout, check_backbone_layers,
                      check_page_attention, check_page_context_dim, check_page_dropout, check_page_encoder, head_layout,
                      page_options)

GAT_MAX_K = engine.GAT_MAX_K
LOSS_MAX_CLASSES = engine.LOSS_MAX_CLASSES

_FIELDS = ("roi_output_size", "n_classes", "use_context", "hidden_dim", "bbox_hidden_dim",
           "n_additional_feat", "drop_prob")


class _ParamBlock(nn.Module):
    """BasicBlock-shaped parameter holder: conv1, bn1, relu, conv2, bn2 (torchvision naming); with ``cin != c`` (layer2's
    block 0) conv1 has stride 2 and a downsample = Sequential(conv 1x1 stride 2, bn) follows."""

    def __init__(self, c, cin=None):
        super().__init__()
        cin = c if cin is None else cin
        stride = 1 if cin == c else 2
        self.conv1 = nn.Conv2d(cin, c, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(c)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(c, c, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(c)
        if cin != c:
            self.downsample = nn.Sequential(nn.Conv2d(cin, c, 1, stride, bias=False), nn.BatchNorm2d(c))

    def forward(self, x):
        raise RuntimeError("parameter container only; the conv stack runs in libcova_hip.so")


class _ParamBottleneck(nn.Module):
    """torchvision Bottleneck-shaped parameter holder (resnet50 layer1; extension): conv1 1x1, bn1,
    conv2 3x3, bn2, conv3 1x1, bn3, relu, optional downsample = Sequential(conv 1x1, bn)."""

    def __init__(self, cin, planes, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * planes)
        self.relu = nn.ReLU(inplace=True)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * planes, 1, bias=False),
                                            nn.BatchNorm2d(4 * planes))

    def forward(self, x):
        raise RuntimeError("parameter container only; the conv stack runs in libcova_hip.so")


class _RoIPoolSpec(nn.Module):
    """Holds (output_size, spatial_scale) like torchvision.ops.RoIPool (models.py:58)."""

    def __init__(self, output_size, spatial_scale):
        super().__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale


def _named_tensors(module):
    params = {k: v for k, v in module.named_parameters()}
    buffers = {k: v for k, v in module.named_buffers()}
    return params, buffers


def _require_cuda(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(
                "cova_web_object_detection_amd runs on MI355X only: got a %s tensor.  Move the model "
                "and its inputs to the ROCm device (there is no CPU fallback)." % t.device)


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def _i64c(t):
    return t.detach().to(torch.int64).contiguous()


def _verify_batch_size(training, n, width):
    """torch.nn.functional.batch_norm's train-mode check (one value per channel has no variance)."""
    if training and n == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size "
                         "torch.Size([1, %d])" % width)


def _layer_modes(model):
    """Each BatchNorm's and Dropout's own ``.training`` ({BatchNorm prefix / Dropout name: bool}, engine.is_train), or
    one bool when they all agree (whole-model train() / eval(): exactly the launches of the single flag)."""
    modes = {}
    for name, m in model.named_modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            modes[name + "."] = m.training
        elif isinstance(m, nn.Dropout):
            modes[name] = m.training
    return engine.collapse_modes(modes) if modes else model.training


def _plan(keys, values, want_dimg):
    """engine.grad_plan of a call whose parameters ``keys``/``values`` follow their own requires_grad; None when
    autograd wants nothing of it (no saved activations, no backward)."""
    if not torch.is_grad_enabled():
        return None
    need = [k for k, v in zip(keys, values) if v.requires_grad]
    if not need and not want_dimg:
        return None
    return engine.grad_plan(need, want_dimg, layer2=any(k.startswith("convnet.5.") for k in keys))


def _only_wanted(ctx, first, keys, grads):
    """Gradients in autograd's order; None for every input that does not require one (frozen parameters)."""
    return tuple(grads.get(k) if ctx.needs_input_grad[first + i] else None for i, k in enumerate(keys))


def _saved_or_raise(sv):
    """The saved activations are released by the first backward (like autograd's saved tensors)."""
    if sv is None:
        raise RuntimeError("Trying to backward through the graph a second time: the saved activations of "
                           "this CoVA forward have already been freed (the HIP path does not support "
                           "retain_graph).")


# ------------------------------------------------------------------------------------- autograd
class _CoVAFn(torch.autograd.Function):
    """Whole forward pass as one autograd node: backward runs engine.model_bwd."""

    @staticmethod
    def forward(ctx, model, modes, plan, images, bboxes, additional_feats, context_indices,
                *param_values):
        keys = model._param_keys
        params = dict(zip(keys, [p.detach() for p in param_values]))
        _, buffers = _named_tensors(model)
        seeds = model._next_dropout_seeds()
        logits, sv = engine.model_fwd(model._cfg, params, buffers, _f32c(images), _f32c(bboxes),
                                      _f32c(additional_feats), _i64c(context_indices),
                                      modes, seeds, model._forced_masks, save=plan is not None, plan=plan)
        ctx.sv, ctx.params, ctx.keys, ctx.plan = sv, params, keys, plan
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        _saved_or_raise(ctx.sv)
        want_dimg = bool(ctx.needs_input_grad[3])            # images.requires_grad (the reference gets it from autograd)
        grads = engine.model_bwd(ctx.sv, dlogits.contiguous(), ctx.params, want_dimg=want_dimg, plan=ctx.plan)
        ctx.sv = None
        return (None, None, None, grads.get("__images__"), None, None, None) + _only_wanted(ctx, 7, ctx.keys, grads)


class _VisualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, modes, plan, images, bboxes, *param_values):
        keys = model._conv_keys
        params = dict(zip(keys, [p.detach() for p in param_values]))
        _, buffers = _named_tensors(model)
        images, bboxes = _f32c(images), _f32c(bboxes)
        feat, sv = engine.convstack_fwd(images, params, buffers, modes, plan is not None and "convstack" in plan)
        out = torch.empty((bboxes.shape[0], model.n_visual_feat), device=images.device)
        if model._cfg["roi_op"] == "align":
            rsv = engine.roialign_fwd(feat, bboxes, model.roi_pool.output_size, model.roi_pool.spatial_scale,
                                      model._cfg["sampling_ratio"], model._cfg["roi_aligned"], out,
                                      model.n_visual_feat)
        else:
            rsv = engine.roipool_fwd(feat, bboxes, model.roi_pool.output_size,
                                     model.roi_pool.spatial_scale, out, model.n_visual_feat)
        ctx.sv, ctx.rsv, ctx.keys, ctx.nv, ctx.params, ctx.plan = sv, rsv, keys, model.n_visual_feat, params, plan
        return out

    @staticmethod
    def backward(ctx, gout):
        bwd = engine.roialign_bwd if ctx.rsv.get("kind") == "align" else engine.roipool_bwd
        gfeat = bwd(ctx.rsv, gout.contiguous(), ctx.nv)
        grads = engine.convstack_bwd(ctx.sv, gfeat, params=ctx.params, want_dimg=bool(ctx.needs_input_grad[3]),
                                     plan=ctx.plan)
        return (None, None, None, grads.get("__images__"), None) + _only_wanted(ctx, 5, ctx.keys, grads)


class _BBoxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, bboxes, *param_values):
        keys = model._bbox_keys
        params = dict(zip(keys, [p.detach() for p in param_values]))
        _, buffers = _named_tensors(model)
        bboxes = _f32c(bboxes)
        out = torch.empty((bboxes.shape[0], model.bbox_hidden_dim), device=bboxes.device)
        ctx.sv = engine.bbox_fwd(bboxes, params, buffers, _layer_modes(model), out, model.bbox_hidden_dim)
        ctx.keys, ctx.hd = keys, model.bbox_hidden_dim
        return out

    @staticmethod
    def backward(ctx, gout):
        grads = engine.bbox_bwd(ctx.sv, gout.contiguous(), ctx.hd)
        return (None, None) + _only_wanted(ctx, 2, ctx.keys, grads)


class _BN1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bn, x, weight, bias):
        x = _f32c(x)
        N, C = x.shape
        params = {"bn.weight": weight.detach(), "bn.bias": bias.detach()}
        buffers = {"bn.running_mean": bn.running_mean, "bn.running_var": bn.running_var,
                   "bn.num_batches_tracked": bn.num_batches_tracked}
        out = torch.empty_like(x)
        ctx.st = engine.bn1d_fwd(x, C, N, C, "bn.", params, buffers, bn.training, out, C, False)
        ctx.x = x
        return out

    @staticmethod
    def backward(ctx, gout):
        x = ctx.x
        N, C = x.shape
        dz = torch.empty_like(x)
        dg, db = engine.bn_backward(gout.contiguous(), C, None, 0, x, C, ctx.st, N, dz, C)
        return (None, dz if ctx.needs_input_grad[1] else None) + _only_wanted(ctx, 2, ("w", "b"), {"w": dg, "b": db})


class _HipBatchNorm1d(nn.BatchNorm1d):
    """nn.BatchNorm1d whose forward/backward run in libcova_hip.so (models.py:73)."""

    def forward(self, x):
        _require_cuda(x)
        if x.dim() != 2 or x.shape[1] != self.num_features:
            raise RuntimeError("expected input [N, %d], got %s" % (self.num_features, tuple(x.shape)))
        if x.shape[0] == 0:
            return x
        _verify_batch_size(self.training, x.shape[0], self.num_features)
        return _BN1dFn.apply(self, x, self.weight, self.bias)


class _GATFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, h_i, context_indices, W_i, W_j, att_w, att_b, edge_w=None, phi=None, drop=None):
        h = _f32c(h_i)
        N, F = h.shape
        params = {"gat.W_i.weight": W_i.detach(), "gat.W_j.weight": W_j.detach(),
                  "gat.attention_layer.weight": att_w.detach(),
                  "gat.attention_layer.bias": att_b.detach()}
        if edge_w is not None:
            params["gat.edge_layer.weight"] = edge_w.detach().contiguous()
        hp = torch.empty((N, layer.hidden_dim), device=h.device)
        ctx.sv = engine.gat_fwd(h, F, N, F, _i64c(context_indices), params, hp, layer.hidden_dim, phi=phi,
                                attention=layer.attention, drop=drop)
        ctx.params = params
        ctx.mark_non_differentiable(ctx.sv["attn"])
        return hp, ctx.sv["attn"]

    @staticmethod
    def backward(ctx, g, _gattn):
        sv = ctx.sv
        dh = torch.empty((sv["N"], sv["F"]), device=g.device)
        grads = engine.gat_bwd(sv, g.contiguous(), sv["D"], ctx.params, dh, sv["F"], False)
        return (None, dh, None, grads["gat.W_i.weight"], grads["gat.W_j.weight"],
                grads["gat.attention_layer.weight"], grads["gat.attention_layer.bias"],
                grads.get("gat.edge_layer.weight"), None, None)


# ------------------------------------------------------------------------------------- modules
def _check_gat_inputs(h_i, context_indices, in_features):
    """What the reference's layer would reject inside torch (models.py:180-200), before raw pointers go out."""
    if h_i.dim() != 2 or h_i.shape[1] != in_features:
        raise RuntimeError("expected h_i [N, %d] (W_i / W_j input width, models.py:161-162), got %s"
                           % (in_features, tuple(h_i.shape)))
    if context_indices.dim() != 2 or context_indices.shape[0] != h_i.shape[0]:
        raise RuntimeError("expected context_indices [%d, n_context], got %s"
                           % (h_i.shape[0], tuple(context_indices.shape)))
    if context_indices.is_floating_point() or context_indices.dtype == torch.bool:
        raise IndexError("context_indices must be an integer tensor (models.py:186 indexes with it)")
    if context_indices.shape[1] > GAT_MAX_K:
        raise ValueError("n_context > %d (-cs > %d) is not supported by the wave-per-node kernel"
                             % (GAT_MAX_K, GAT_MAX_K // 2))


def _edge_features(context_indices, bboxes, page_size):
    """phi [N, K, 8] of one batch for the edge-aware layers (engine.edge_geometry); ValueError without boxes / page size."""
    if bboxes is None or page_size is None:
        raise ValueError("an edge-aware GraphAttentionLayer (edge_geometry=True) needs bboxes [N, 5] and "
                         "page_size = (height, width)")
    _require_cuda(bboxes)
    if bboxes.dim() != 2 or bboxes.shape[1] != 5 or bboxes.shape[0] != context_indices.shape[0]:
        raise RuntimeError("expected bboxes [%d, 5], got %s" % (context_indices.shape[0], tuple(bboxes.shape)))
    return engine.edge_geometry(_f32c(bboxes), _i64c(context_indices), page_size)


class GraphAttentionLayer(nn.Module):
    """Single-head additive attention over K padded neighbours (reference models.py:151-212).
    ``edge_geometry=True`` (extension): the score of an edge also takes ``edge_layer`` (Linear(8, 1), no bias, zero at
    construction) of its relative-geometry features (include/cova_hip.h, cova_edge_geometry).
    ``attention="gatv2"`` (extension): the dynamic score of Brody et al. (ICLR 2022), ``attention_layer(LeakyReLU(W_i h_i +
    W_j h_j))`` with ``attention_layer`` a Linear(hidden_dim, 1), instead of the reference's static
    ``LeakyReLU(attention_layer([W_i h_i ; W_j h_j]))``; the edge term is then added outside the non-linearity.
    ``attention_dropout=p`` (extension, 0 <= p < 1): inverted dropout on the normalised attention coefficients while the
    layer (its ``attn_drop`` submodule) is in train mode (GAT paper, section 3.3; PyG ``GATConv(dropout=)``, DGL
    ``attn_drop``).  The weights returned with ``return_attn_wts`` stay the distribution before dropout.  The masks are
    regenerated in the kernels from a per-call seed (seed_dropout); with p = 0 no submodule is created."""

    def __init__(self, in_features, hidden_dim, alpha=0.2, edge_geometry=False, attention="gat", attention_dropout=0.0):
        super(GraphAttentionLayer, self).__init__()
        if abs(alpha - engine.LEAKY_SLOPE) > 1e-12:
            raise ValueError("the HIP path is built for the reference's LeakyReLU slope 0.2")
        self.in_features = in_features
        self.hidden_dim = hidden_dim
        self.edge_geometry = bool(edge_geometry)
        self.attention = check_attention(attention)
        self.attention_dropout = check_attention_dropout(attention_dropout)
        self._dropout_seed, self._dropout_calls = 0x5EED, 0
        self.W_i = nn.Linear(self.in_features, self.hidden_dim, bias=False)
        self.W_j = nn.Linear(self.in_features, self.hidden_dim, bias=False)
        self.attention_layer = nn.Linear((1 if self.attention == "gatv2" else 2) * self.hidden_dim, 1)
        self.leakyrelu = nn.LeakyReLU(alpha)
        if self.edge_geometry:
            self.edge_layer = nn.Linear(EDGE_FEATURES, 1, bias=False)
            nn.init.zeros_(self.edge_layer.weight)
        if self.attention_dropout > 0:
            self.attn_drop = nn.Dropout(self.attention_dropout)     # rate and train / eval mode (no weights; never called)

    def seed_dropout(self, seed):
        """Seed of the attention-dropout masks of a layer called on its own (inside CoVA / MultiHeadGraphAttention the
        owner's seed governs): call c (1, 2, ...) draws from engine.attention_dropout_seed(engine.dropout_base(seed, c), 0, 0)."""
        self._dropout_seed, self._dropout_calls = int(seed), 0

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        w = state_dict.get(prefix + "attention_layer.weight")
        if torch.is_tensor(w) and w.shape != self.attention_layer.weight.shape:
            try:
                theirs = "attention=%r" % attention_of(w, self.hidden_dim, prefix)
            except ValueError:
                theirs = "neither attention mode at hidden_dim %d" % self.hidden_dim
            error_msgs.append("%sattention_layer.weight: this layer was built with attention=%r (weight %s), the "
                              "checkpoint's %s belongs to %s; a checkpoint loads into the attention mode it was trained "
                              "with only" % (prefix, self.attention, tuple(self.attention_layer.weight.shape),
                                             tuple(w.shape), theirs))
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, h_i, context_indices, return_attn_wts=False, bboxes=None, page_size=None, phi=None, drop_seed=None):
        """h_i [N, in_features]; context_indices int64 [N, n_context] with -1 pads.  An edge-aware layer also needs
        ``bboxes`` [N, 5] and ``page_size`` = (height, width), or the ``phi`` [N, n_context, 8] computed from them.
        ``drop_seed``: the attention-dropout stream of this call (MultiHeadGraphAttention hands each head its own)."""
        _require_cuda(h_i, context_indices)
        _check_gat_inputs(h_i, context_indices, self.in_features)
        drop = None
        if self.attention_dropout > 0 and self.attn_drop.training:
            if drop_seed is None:
                self._dropout_calls += 1
                drop_seed = engine.attention_dropout_seed(engine.dropout_base(self._dropout_seed, self._dropout_calls), 0, 0)
            drop = (self.attention_dropout, int(drop_seed))
        if not self.edge_geometry:
            h_prime, attn = _GATFn.apply(self, h_i, context_indices, self.W_i.weight, self.W_j.weight,
                                         self.attention_layer.weight, self.attention_layer.bias, None, None, drop)
        else:
            if phi is None:
                phi = _edge_features(context_indices, bboxes, page_size)
            h_prime, attn = _GATFn.apply(self, h_i, context_indices, self.W_i.weight, self.W_j.weight,
                                         self.attention_layer.weight, self.attention_layer.bias,
                                         self.edge_layer.weight, phi, drop)
        if return_attn_wts:
            return h_prime, attn
        return h_prime


class _GATHeads(nn.Module):
    def __init__(self, in_features, hidden_dim, n_heads, edge_geometry=False, attention="gat", attention_dropout=0.0):
        super().__init__()
        self.heads = nn.ModuleList([GraphAttentionLayer(in_features, hidden_dim // n_heads, edge_geometry=edge_geometry,
                                                        attention=attention, attention_dropout=attention_dropout)
                                    for _ in range(n_heads)])


class MultiHeadGraphAttention(nn.Module):
    """Extension (BASELINE.json configs[2], [4]; the reference has one single-head layer,
    models.py:78-79): ``n_layers`` stacked layers, each the concatenation of ``n_heads``
    GraphAttentionLayers of hidden_dim/n_heads channels over the same neighbour table.  Same call
    contract as GraphAttentionLayer; the attention weights returned are the last layer's, per head
    [N, n_heads, n_context].  ``edge_geometry``: every head is edge-aware; the features are computed once per call.
    ``attention``: the scoring mode of every head ('gat' | 'gatv2', GraphAttentionLayer).
    ``attention_dropout``: every head drops attention coefficients (GraphAttentionLayer) from a stream of its own,
    engine.attention_dropout_seed(base, layer, head), ``base`` = engine.dropout_base(seed, call) of seed_dropout()."""

    def __init__(self, in_features, hidden_dim, n_heads, n_layers, edge_geometry=False, attention="gat",
                 attention_dropout=0.0):
        super().__init__()
        if hidden_dim % n_heads:
            raise ValueError("hidden_dim must be divisible by n_heads")
        self.edge_geometry = bool(edge_geometry)
        self.attention = check_attention(attention)
        self.attention_dropout = check_attention_dropout(attention_dropout)
        self._dropout_seed, self._dropout_calls = 0x5EED, 0
        self.layers = nn.ModuleList([_GATHeads(in_features if l == 0 else hidden_dim, hidden_dim, n_heads, edge_geometry,
                                               attention, self.attention_dropout) for l in range(n_layers)])

    def seed_dropout(self, seed):
        self._dropout_seed, self._dropout_calls = int(seed), 0

    def forward(self, h_i, context_indices, return_attn_wts=False, bboxes=None, page_size=None, phi=None):
        h, attn, base = h_i, None, None
        if self.attention_dropout > 0:
            self._dropout_calls += 1
            base = engine.dropout_base(self._dropout_seed, self._dropout_calls)
        if self.edge_geometry and phi is None:
            _require_cuda(h_i, context_indices)
            phi = _edge_features(context_indices, bboxes, page_size)
        for l, layer in enumerate(self.layers):
            outs = [head(h, context_indices, True, phi=phi,
                         drop_seed=None if base is None else engine.attention_dropout_seed(base, l, i))
                    for i, head in enumerate(layer.heads)]
            h = torch.cat([o for o, _ in outs], dim=1)
            attn = torch.stack([a for _, a in outs], dim=1)
        return (h, attn) if return_attn_wts else h


class _PageLayerFn(torch.autograd.Function):
    """The one autograd node of the page modules (_PageLayer): ``layer`` names its state_dict prefix, the engine forward /
    backward pair and which saved tensor, if any, is the non-differentiable second output; ``values`` are its parameters
    in named_parameters() order."""

    @staticmethod
    def forward(ctx, layer, h, page_start, bboxes, page_size, *values):
        h = _f32c(h)
        ctx.keys = [layer._prefix + k for k, _ in layer.named_parameters()]
        ctx.params = {k: _f32c(v) for k, v in zip(ctx.keys, values)}
        out = torch.empty((h.shape[0], layer.dim), device=h.device)
        ctx.sv = layer._engine_fwd(h, _i64c(page_start), ctx.params, out, _f32c(bboxes) if layer.geometry_bias else None,
                                   page_size)
        ctx.bwd = layer._engine_bwd
        if layer._second is None:
            return out
        ctx.mark_non_differentiable(ctx.sv[layer._second])
        return out, ctx.sv[layer._second]

    @staticmethod
    def backward(ctx, g, _gsecond=None):
        sv = ctx.sv
        dh = torch.zeros((sv["N"], sv["F"]), device=g.device)          # the engine's page backwards accumulate
        grads = ctx.bwd(sv, g.contiguous(), g.shape[1], ctx.params, dh, sv["F"])
        return (None, dh, None, None, None) + tuple(grads[k] for k in ctx.keys)


class _PageLayer(nn.Module):
    """What PageReadout, PageAttention and PageEncoder share: the input checks, the autograd node and, for the two layers
    that have one, the dropout of a module called on its own."""
    _prefix = _second = _drop_name = None
    geometry_bias = False
    dropout = 0.0
    _dropout_seed, _dropout_calls = 0x5EED, 0

    def _init_dropout(self, p, option):
        """The layer's rate; with p > 0 its weightless nn.Dropout submodule ``_drop_name`` (rate and train / eval mode;
        never called)."""
        self.dropout = check_page_dropout(p, option)
        if self.dropout > 0:
            setattr(self, self._drop_name, nn.Dropout(self.dropout))

    def seed_dropout(self, seed):
        """Seed of the dropout masks of a layer called on its own (inside CoVA the model's seed governs): call c (1, 2, ...)
        that drops draws from engine.page_dropout_seed(engine.dropout_base(seed, c), layer, site)."""
        self._dropout_seed, self._dropout_calls = int(seed), 0

    def _drop_args(self):
        """dropout=, seed_base= and training= of the engine forward for this call."""
        if self.dropout > 0 and getattr(self, self._drop_name).training:
            self._dropout_calls += 1
            return dict(dropout=self.dropout, seed_base=engine.dropout_base(self._dropout_seed, self._dropout_calls),
                        training=True)
        return dict(dropout=0.0, seed_base=0, training=False)

    def _run(self, h, page_start, bboxes=None, page_size=None):
        """The node's output(s) for checked inputs; None for an empty batch (the caller shapes its empty result)."""
        _require_cuda(h, page_start)
        if self.geometry_bias:
            if bboxes is None or page_size is None or bboxes.dim() != 2 or tuple(bboxes.shape) != (h.shape[0], 5):
                raise ValueError("a %s with geometry=True needs bboxes [N, 5] and page_size = (height, width)"
                                 % type(self).__name__)
            _require_cuda(bboxes)
        if h.dim() != 2 or h.shape[1] != self.in_features:
            raise RuntimeError("expected h [N, %d], got %s" % (self.in_features, tuple(h.shape)))
        if page_start.dim() != 1 or page_start.shape[0] < 1 or page_start.is_floating_point():
            raise ValueError("page_start must hold B + 1 integer row offsets, got shape %s" % (tuple(page_start.shape),))
        if h.shape[0] == 0:
            return None
        return _PageLayerFn.apply(self, h, page_start, bboxes, page_size, *self.parameters())


class PageReadout(_PageLayer):
    """Extension: the global-attention readout of Li et al. 2016 (gated graph networks; PyG ``AttentionalAggregation``)
    over the boxes of each page.  ``P = W h`` (Linear(in_features, dim), no bias), ``beta`` = softmax over the page's boxes
    of ``LeakyReLU(attention_layer(P))`` (Linear(dim, 1)), ``r_p = sum beta_i P_i``; every box of a page receives its
    page's ``r_p``.  ``forward(h [N, in_features], page_start int64 [B + 1])`` -> ``r_rows [N, dim]`` (and ``beta [N]`` with
    ``return_attn_wts``); one autograd node over cova_page_readout_fwd / cova_page_readout_bwd."""

    _prefix, _second, _engine_bwd = "page_readout.", "beta", staticmethod(engine.page_readout_bwd)

    def __init__(self, in_features, dim, alpha=0.2):
        super().__init__()
        if abs(alpha - engine.LEAKY_SLOPE) > 1e-12:
            raise ValueError("the HIP path is built for the reference's LeakyReLU slope 0.2")
        self.in_features, self.dim = in_features, check_page_context_dim(dim)
        if self.dim < 1:
            raise ValueError("PageReadout needs dim >= 1")
        self.W = nn.Linear(in_features, self.dim, bias=False)
        self.attention_layer = nn.Linear(self.dim, 1)

    def _engine_fwd(self, h, page_start, params, out, bboxes, page_size):
        return engine.page_readout_fwd(h, h.shape[1], h.shape[0], h.shape[1], page_start, params, out, self.dim)

    def forward(self, h, page_start, return_attn_wts=False):
        out, beta = self._run(h, page_start) or (h.new_empty((0, self.dim)), h.new_empty((0,)))
        return (out, beta) if return_attn_wts else out


class PageAttention(_PageLayer):
    """Extension: multi-head scaled dot-product self-attention (Vaswani et al. 2017) restricted to pages.  ``[Q | K | V] =
    qkv(h)`` (Linear(in_features, 3 dim), no bias); for a box i and a head of ``dim / heads`` columns, ``A_ij`` = softmax
    over ALL boxes j of i's page of ``Q_i . K_j / sqrt(dim / heads)`` and ``O_i = sum_j A_ij V_j``.  No output projection
    (the decoder's first Linear follows).  ``forward(h [N, in_features], page_start int64
    [B + 1])`` -> ``O [N, dim]`` (and ``lse [N, heads]``, the log-sum-exp of each row's scores, with ``return_lse``); one
    autograd node over cova_page_attn_fwd / cova_page_attn_bwd.
    ``geometry=True`` (extension; the relative 2-D bias of LayoutLMv2, Xu et al. 2021, on this project's own features):
    the score of a pair also takes ``geometry`` (Linear(8, heads), no bias, zero at construction: the fresh layer computes
    the plain layer's output) of the eight relative-geometry features of cova_edge_geometry, query box against key box,
    formed inside the kernels (cova_page_attn_fwd_geo / cova_page_attn_bwd_geo).  ``forward`` then needs ``bboxes``
    [N, 5] and ``page_size`` = (height, width) in pixels; the boxes get no gradient.
    ``dropout=p`` (extension, 0 <= p < 1; the ``dropout`` of nn.MultiheadAttention): inverted dropout on the probabilities
    ``A`` while the layer's ``attn_drop`` submodule (a weightless nn.Dropout, created only when p > 0) is in train mode,
    ``O_i = sum_j D_ij A_ij V_j / (1 - p)``; ``lse`` stays the undropped one.  No mask is stored: the kernels regenerate it
    from a per-call seed (seed_dropout; cova_page_attn_fwd_drop / cova_page_attn_bwd_drop).  The GAT's ``attention_dropout``
    does not reach this layer."""

    _prefix, _second, _engine_bwd = "page_attention.", "lse", staticmethod(engine.page_attn_bwd)
    _drop_name = "attn_drop"

    def __init__(self, in_features, dim, heads=1, geometry=False, dropout=0.0):
        super().__init__()
        self.in_features = in_features
        self.dim, self.heads = check_page_attention(dim, heads)
        if self.dim < 1:
            raise ValueError("PageAttention needs dim >= 4")
        self.qkv = nn.Linear(in_features, 3 * self.dim, bias=False)
        self.geometry_bias = bool(geometry)
        if self.geometry_bias:
            self.geometry = nn.Linear(8, self.heads, bias=False)
            nn.init.zeros_(self.geometry.weight)
        self._init_dropout(dropout, PAGE_ATTENTION_DROPOUT_OPTION)

    def _engine_fwd(self, h, page_start, params, out, bboxes, page_size):
        return engine.page_attn_fwd(h, h.shape[1], h.shape[0], h.shape[1], page_start, params, self.heads, out, self.dim,
                                    bboxes=bboxes, page_size=page_size, **self._drop_args())

    def forward(self, h, page_start, bboxes=None, page_size=None, return_lse=False):
        out, lse = (self._run(h, page_start, bboxes, page_size)
                    or (h.new_empty((0, self.dim)), h.new_empty((0, self.heads))))
        return (out, lse) if return_lse else out


class _PageEncoderBlock(nn.Module):
    """Parameter holder of one pre-LN block: norm1, qkv, (geometry,) out, norm2, ffn1, ffn2 in state_dict order."""

    def __init__(self, dim, heads, ffn_dim, geometry):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.qkv = nn.Linear(dim, 3 * dim, bias=False)
        if geometry:
            self.geometry = nn.Linear(8, heads, bias=False)
            nn.init.zeros_(self.geometry.weight)
        self.out = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim)
        self.ffn1 = nn.Linear(dim, ffn_dim)
        self.ffn2 = nn.Linear(ffn_dim, dim)

    def forward(self, x):
        raise RuntimeError("parameter container only; the block runs in libcova_hip.so (PageEncoder.forward)")


class PageEncoder(_PageLayer):
    """Extension: an L-layer pre-LN transformer encoder (Vaswani et al. 2017; the pre-LN form of Xiong et al. 2020) over
    the boxes of each page -- torch's ``nn.TransformerEncoderLayer(norm_first=True, activation="gelu", dropout=p)`` per
    page with a zero ``in_proj_bias``, behind an input projection and in front of a final LayerNorm:
        x = input(h)                                  Linear(in_features, dim), no bias (a LayerNorm follows)
        per layer:  x = x + out(page attention of qkv(norm1(x)));   x = x + ffn2(GELU(ffn1(norm2(x))))
        return norm(x)
    The attention is PageAttention's (every box attends to ALL boxes of its page, ``heads`` heads, cova_page_attn_fwd);
    ``geometry=True`` gives every layer the box-geometry bias of PageAttention(geometry=True) (``layers.<l>.geometry``,
    Linear(8, heads), no bias, zero at construction; ``forward`` then needs ``bboxes`` [N, 5] and ``page_size`` = (height,
    width)).  GELU is the exact (erf) form, eps = 1e-5.  The GAT's ``attention_dropout`` and ``edge_geometry`` do not
    reach the encoder.
    ``dropout=p`` (0 <= p < 1; torch's single ``dropout`` argument, default 0 here): while the encoder's ``drop`` submodule (a
    weightless nn.Dropout, created only when p > 0) is in train mode every block runs
        x = x + drop1(out(page attention with dropped probabilities));   x = x + drop2(ffn2(drop_h(GELU(ffn1(norm2(x))))))
    four sites per layer, each on a stream of its own (engine.page_dropout_seed), none on the input projection or the
    final LayerNorm.  No mask is stored: the kernels regenerate them from a per-call seed (seed_dropout).
    ``forward(h [N, in_features], page_start int64 [B + 1])``
    -> ``[N, dim]``; one autograd node over engine.page_encoder_fwd / page_encoder_bwd (cova_layernorm_*, cova_gelu_*,
    cova_page_attn_*, cova_sgemm, cova_colsum; with dropout cova_dropout_add_fwd / cova_dropout_regen_bwd and the _drop
    forms)."""

    _prefix, _engine_bwd = "page_encoder.", staticmethod(engine.page_encoder_bwd)
    _drop_name = "drop"

    def __init__(self, in_features, dim, heads=1, layers=1, ffn_dim=None, geometry=False, dropout=0.0):
        super().__init__()
        self.in_features = in_features
        self.dim, self.heads, self.n_layers, self.ffn_dim, self.geometry_bias = check_page_encoder(dim, heads, layers,
                                                                                                   ffn_dim, geometry)
        if self.dim < 1:
            raise ValueError("PageEncoder needs dim >= 4")
        self.input = nn.Linear(in_features, self.dim, bias=False)
        self.layers = nn.ModuleList(_PageEncoderBlock(self.dim, self.heads, self.ffn_dim, self.geometry_bias)
                                    for _ in range(self.n_layers))
        self.norm = nn.LayerNorm(self.dim)
        self._init_dropout(dropout, PAGE_ENCODER_DROPOUT_OPTION)

    def _engine_fwd(self, h, page_start, params, out, bboxes, page_size):
        return engine.page_encoder_fwd(h, h.shape[1], h.shape[0], h.shape[1], page_start, params, self.heads, self.n_layers,
                                       out, self.dim, bboxes=bboxes, page_size=page_size, **self._drop_args())

    def forward(self, h, page_start, bboxes=None, page_size=None):
        out = self._run(h, page_start, bboxes, page_size)
        return h.new_empty((0, self.dim)) if out is None else out


class CoVA(nn.Module):
    def __init__(self, roi_output_size, img_H, n_classes, use_context=True, hidden_dim=384,
                 bbox_hidden_dim=32, n_additional_feat=0, drop_prob=0.2, class_names=None,
                 backbone="resnet18", n_heads=1, n_gat_layers=1, backbone_state_dict=None, roi_op="pool",
                 sampling_ratio=2, roi_aligned=False, backbone_layers=1, edge_geometry=False, attention="gat",
                 attention_dropout=0.0, page_context_dim=0, page_attention_dim=0, page_attention_heads=1,
                 page_attention_geometry=False, page_encoder_dim=0, page_encoder_heads=1, page_encoder_layers=1,
                 page_encoder_ffn_dim=None, page_encoder_geometry=False, page_attention_dropout=0.0,
                 page_encoder_dropout=0.0):
        """The first nine arguments exactly as the reference's CoVA (models.py:10-34; called positionally
        at main.py:122-132).  Keyword-only-in-practice extensions, whose defaults are the reference's
        model: ``backbone`` 'resnet18' | 'resnet50' (torchvision ``children()[:-5]`` of either),
        ``n_heads`` / ``n_gat_layers`` (MultiHeadGraphAttention), ``backbone_state_dict`` = a torchvision
        ResNet state_dict (or a path to one) whose conv1 / bn1 / layer1 entries initialise the stack --
        the offline stand-in for the reference's ``pretrained=True`` download (models.py:49).
        ``roi_op='align'`` swaps RoIPool (the reference's operator and the parity path) for torchvision's RoIAlign
        (``sampling_ratio``, ``roi_aligned`` as in ``torchvision.ops.RoIAlign``).
        ``img_H`` is only used for the RoIPool scale (models.py:53-56): pages may be any H x W.
        ``backbone_layers=2`` (resnet18 only) keeps torchvision's ``layer2`` after layer1 (``children()[:-4]``): 128
        channels at stride 8, parameters under ``convnet.5.``.
        ``edge_geometry=True``: every attention head scores an edge with its relative box geometry as well (one
        ``edge_layer.weight`` [1, 8] per head, zero at construction: the fresh model computes the plain model's output);
        the page size is taken from ``images``.
        ``attention="gatv2"``: every head scores with the GATv2 form ``a . LeakyReLU(W_i h_i + W_j h_j) + b`` (dynamic
        attention: the ranking of a box's neighbours depends on the box); ``attention_layer.weight`` is then
        [1, hidden_dim / n_heads], so checkpoints of the two modes do not load into each other.
        ``attention_dropout=p`` (0 <= p < 1): dropout on the attention coefficients of every head in train mode
        (GraphAttentionLayer); the masks follow seed_dropout() like the decoder's, from streams of their own.  No weights:
        the state_dict is unchanged; with p = 0 the module list is too.
        ``page_context_dim=G`` (0 <= G <= 512; independent of ``use_context``): a PageReadout of the own features gives every
        box G more columns, the attention-pooled vector of its page (``page_readout.*``, between ``gat`` and ``decoder``
        in the state_dict); the pages are read off the page column of ``bboxes`` and the page count of ``images``.  With 0 the
        module list, the state_dict and every launch are unchanged.
        ``page_attention_dim=E`` with ``page_attention_heads=Hh`` (0 <= E <= 512, Hh divides E, E / Hh a multiple of 4 in
        [4, 128]; independent of ``use_context`` and of ``page_context_dim``): a PageAttention of the own features gives
        every box E more columns behind the readout's, its own attention-weighted view of ALL boxes of its page
        (``page_attention.qkv.weight``, between ``page_readout`` and ``decoder`` in the state_dict).  ``edge_geometry`` and
        ``attention_dropout`` belong to the GAT and do not reach this layer (``page_attention_dropout`` does).  With 0 nothing
        changes.
        ``page_attention_geometry=True`` (needs ``page_attention_dim`` > 0, else ValueError): the page attention's scores
        take a bias from the relative geometry of the two boxes (``page_attention.geometry.weight`` [Hh, 8], zero at
        construction, directly behind ``page_attention.qkv.weight``); the page size is taken from ``images``.
        ``page_encoder_dim=P`` (0 <= P <= 512, 0 = off; independent of ``use_context``, ``page_context_dim`` and
        ``page_attention_dim``): a PageEncoder of the own features -- ``page_encoder_layers`` (1..8) pre-LN transformer
        blocks of ``page_encoder_heads`` heads (the page attention's rule for P / Hh) and a feed-forward width
        ``page_encoder_ffn_dim`` (a multiple of 4 in [4, 2048]; None: 2 P) -- gives every box P more columns behind the page
        attention's (``page_encoder.*``, between ``page_attention`` and ``decoder`` in the state_dict).
        ``page_encoder_geometry=True`` (needs P > 0) gives every layer's scores the box-geometry bias
        (``page_encoder.layers.<l>.geometry.weight`` [Hh, 8], zero at construction).  ``edge_geometry`` and
        ``attention_dropout`` belong to the GAT and do not reach it.  With 0 nothing changes.
        ``page_attention_dropout=p`` (0 <= p < 1; needs ``page_attention_dim`` > 0, else ValueError): dropout on the page
        attention's probabilities in train mode (PageAttention(dropout=), submodule ``page_attention.attn_drop``).
        ``page_encoder_dropout=p`` (0 <= p < 1; needs ``page_encoder_dim`` > 0): torch's ``dropout=`` of
        nn.TransformerEncoderLayer on the four sites of every encoder block (PageEncoder(dropout=), submodule
        ``page_encoder.drop``).  Both follow seed_dropout() like the decoder's masks, from streams of their own
        (engine.page_dropout_seed); no mask is stored, no weights: the state_dict is unchanged, and with p = 0 the module
        list and every launch are too."""
        page = page_options(locals())
        check_backbone_layers(backbone, backbone_layers)
        check_attention(attention)
        attention_dropout = check_attention_dropout(attention_dropout)
        if roi_op not in ("pool", "align"):
            raise ValueError("roi_op must be 'pool' (the reference, models.py:58) or 'align'")
        super(CoVA, self).__init__()
        self.n_classes = n_classes
        self.use_context = use_context
        self.hidden_dim = hidden_dim
        self.bbox_hidden_dim = bbox_hidden_dim
        self.n_additional_feat = n_additional_feat
        self.class_names = (np.arange(self.n_classes).astype(str) if class_names is None
                            else class_names)
        roi_output_size = (int(roi_output_size[0]), int(roi_output_size[1]))

        # ---- representation network.  ImageNet weights (models.py:49 pretrained=True) cannot be
        # fetched offline: convs get torchvision's kaiming-normal(fan_out) init unless a torchvision
        # state_dict is supplied (the explicit backbone_state_dict= argument: a dict or a path; no hidden
        # environment state) or a reference checkpoint is loaded afterwards with load_state_dict.
        c = engine.C64
        c_out = backbone_channels(backbone, backbone_layers)
        conv1 = nn.Conv2d(3, c, 7, 2, 3, bias=False)
        if backbone == "resnet18":
            layer1 = nn.Sequential(_ParamBlock(c), _ParamBlock(c))
        else:
            layer1 = nn.Sequential(_ParamBottleneck(c, c, True), _ParamBottleneck(c_out, c, False),
                                   _ParamBottleneck(c_out, c, False))
        self.backbone, self.backbone_layers = backbone, backbone_layers
        stages = [layer1]
        if backbone_layers == 2:
            stages.append(nn.Sequential(_ParamBlock(c_out, c), _ParamBlock(c_out)))
        self.convnet = nn.Sequential(conv1, nn.BatchNorm2d(c), nn.ReLU(inplace=True),
                                     nn.MaxPool2d(3, 2, 1), *stages)
        for m in self.convnet.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self._init_backbone(backbone_state_dict)
        c = c_out
        # models.py:53-56 reads the output size off a dummy forward; it is a closed form
        feat_h = engine.feature_map_size(img_H, backbone_layers)
        self.roi_pool = _RoIPoolSpec(roi_output_size, feat_h / img_H)
        self.n_visual_feat = c * roi_output_size[0] * roi_output_size[1]
        self.n_feat = self.n_visual_feat + self.bbox_hidden_dim + self.n_additional_feat

        if self.bbox_hidden_dim > 0:
            self.bbox_feat_encoder = nn.Sequential(nn.Linear(5, self.bbox_hidden_dim),
                                                   nn.BatchNorm1d(self.bbox_hidden_dim), nn.ReLU())
        if self.n_additional_feat > 0:
            self.bn_additional_feat = _HipBatchNorm1d(self.n_additional_feat)
        else:
            self.bn_additional_feat = lambda x: x

        if self.use_context:
            if n_heads == 1 and n_gat_layers == 1:
                self.gat = GraphAttentionLayer(self.n_feat, self.hidden_dim, edge_geometry=edge_geometry,
                                               attention=attention, attention_dropout=attention_dropout)
            else:
                self.gat = MultiHeadGraphAttention(self.n_feat, self.hidden_dim, n_heads, n_gat_layers, edge_geometry,
                                                   attention, attention_dropout)
        self.page_context_dim = page["page_context_dim"]
        if self.page_context_dim > 0:
            self.page_readout = PageReadout(self.n_feat, self.page_context_dim)
        self.page_attention_dim, self.page_attention_heads = page["page_attention_dim"], page["page_attention_heads"]
        if self.page_attention_dim > 0:
            self.page_attention = PageAttention(self.n_feat, self.page_attention_dim, self.page_attention_heads,
                                                geometry=page["page_attention_geometry"],
                                                dropout=page[PAGE_ATTENTION_DROPOUT_OPTION])
        self.page_encoder_dim = page["page_encoder_dim"]
        if self.page_encoder_dim > 0:
            self.page_encoder = PageEncoder(self.n_feat, *(page[k] for k in PAGE_ENCODER_OPTIONS),
                                            dropout=page[PAGE_ENCODER_DROPOUT_OPTION])
        self._cfg = dict(roi_output_size=roi_output_size, n_classes=n_classes, use_context=use_context,
                         hidden_dim=hidden_dim, bbox_hidden_dim=bbox_hidden_dim,
                         n_additional_feat=n_additional_feat, drop_prob=float(drop_prob),
                         spatial_scale=self.roi_pool.spatial_scale, backbone=backbone,
                         n_heads=n_heads, n_gat_layers=n_gat_layers, roi_op=roi_op,
                         sampling_ratio=int(sampling_ratio), roi_aligned=bool(roi_aligned),
                         backbone_layers=backbone_layers, edge_geometry=bool(edge_geometry) and bool(use_context),
                         attention=attention, attention_dropout=attention_dropout if use_context else 0.0, **page)
        self.n_total_feat = head_layout(self._cfg, self.n_visual_feat).T
        self.decoder = nn.Sequential(nn.Dropout(drop_prob),
                                     nn.Linear(self.n_total_feat, self.n_total_feat),
                                     nn.BatchNorm1d(self.n_total_feat), nn.ReLU(),
                                     nn.Dropout(drop_prob),
                                     nn.Linear(self.n_total_feat, self.n_classes))

        self._param_keys = [k for k, _ in self.named_parameters()]
        self._conv_keys = [k for k in self._param_keys if k.startswith("convnet.")]
        self._bbox_keys = [k for k in self._param_keys if k.startswith("bbox_feat_encoder.")]
        self._dropout_seed, self._dropout_calls = 0x5EED, 0
        self._forced_masks = None      # parity tests inject keep-masks here
        print("Model Parameters:", sum(p.numel() for p in self.parameters() if p.requires_grad))

    _warned_random_init = set()

    def _init_backbone(self, source):
        """conv1 / bn1 / layer1 of a torchvision ResNet state_dict -> convnet.0 / .1 / .4 (keys map 1:1).
        Without one the stack keeps its random init, which the reference never does: say so."""
        if source is None:
            if self.backbone not in CoVA._warned_random_init:          # once per process and architecture
                CoVA._warned_random_init.add(self.backbone)
                warnings.warn("CoVA: no ImageNet weights for the %s stack (the reference downloads them, "
                              "models.py:49); it starts from a random init.  Pass backbone_state_dict= (a torchvision "
                              "state_dict or a path to one), or load a checkpoint." % self.backbone, stacklevel=3)
            return
        if isinstance(source, (str, bytes, os.PathLike)):
            print("CoVA: backbone weights from", source)
            sd = torch.load(source, map_location="cpu")
        else:
            sd = source
        mapped = {}
        for k, v in sd.items():
            for src, dst in (("conv1.", "0."), ("bn1.", "1."), ("layer1.", "4."), ("layer2.", "5."))[:3 + (
                    self.backbone_layers == 2)]:
                if k.startswith(src):
                    mapped[dst + k[len(src):]] = v
        missing = self.convnet.load_state_dict(mapped, strict=True)
        assert not missing.missing_keys

    # ---------------------------------------------------------------- dropout randomness
    def seed_dropout(self, seed):
        self._dropout_seed, self._dropout_calls = int(seed), 0

    def _next_dropout_seeds(self):
        self._dropout_calls += 1
        base = (self._dropout_seed * 0x9E3779B1 + self._dropout_calls * 2) & 0xFFFFFFFFFFFF
        return base, base + 1

    # ---------------------------------------------------------------- reference surface
    def forward(self, images, bboxes, additional_feats, context_indices):
        """images [B,3,H,W] f32, bboxes [N,5] f32 = [batch_idx,x1,y1,x2,y2], additional_feats
        [N,A] f32, context_indices int64 [N,K] (-1 pads) -> scores [N,n_classes] (models.py:94-122)."""
        _require_cuda(images, bboxes, additional_feats, context_indices)
        modes = _layer_modes(self)
        engine.check_batch(self._cfg, images, bboxes, additional_feats, context_indices, modes)
        if bboxes.shape[0] == 0:
            return torch.empty((0, self.n_classes), device=images.device)
        values = [p for _, p in self.named_parameters()]
        plan = _plan(self._param_keys, values, images.requires_grad)
        return _CoVAFn.apply(self, modes, plan, images, bboxes, additional_feats, context_indices,
                             *values)

    def _get_visual_features(self, images, bboxes):
        _require_cuda(images, bboxes)
        if images.dim() != 4 or images.shape[1] != 3 or bboxes.dim() != 2 or bboxes.shape[1] != 5:
            raise RuntimeError("expected images [B, 3, H, W] and bboxes [N, 5], got %s and %s"
                               % (tuple(images.shape), tuple(bboxes.shape)))
        named = dict(self.named_parameters())
        values = [named[k] for k in self._conv_keys]
        plan = _plan(self._conv_keys, values, images.requires_grad)
        return _VisualFn.apply(self, _layer_modes(self), plan, images, bboxes, *values)

    def _get_bbox_features(self, bboxes):
        """[x,y,w,h,asp_ratio] -> Linear -> BN -> ReLU (models.py:129-148)."""
        if self.bbox_hidden_dim > 0:
            _require_cuda(bboxes)
            if bboxes.dim() != 2 or bboxes.shape[1] != 5:
                raise RuntimeError("expected bboxes [N, 5], got %s" % (tuple(bboxes.shape),))
            _verify_batch_size(self.bbox_feat_encoder[1].training, bboxes.shape[0], self.bbox_hidden_dim)
            named = dict(self.named_parameters())
            return _BBoxFn.apply(self, bboxes, *[named[k] for k in self._bbox_keys])
        return bboxes[:, :0]


# ------------------------------------------------------------------------------------- criterion
class _CELossFn(torch.autograd.Function):
    """cova_ce_loss_fwd + cova_ce_loss_bwd as one autograd node (gradient with respect to the logits only)."""

    @staticmethod
    def forward(ctx, logits, labels, weight, opts):
        lg, lb = _f32c(logits), _i64c(labels)
        acc, _ = engine.ce_loss_fwd(lg, lb, weight, opts, want_pred=False)
        loss, _ = engine.ce_loss_bwd(lg, lb, weight, opts, acc, want_grad=False)
        ctx.save_for_backward(lg, lb, acc)
        ctx.weight, ctx.opts = weight, opts
        return loss[0]

    @staticmethod
    def backward(ctx, grad):
        lg, lb, acc = ctx.saved_tensors
        # the incoming scalar gradient stays on the device: the kernel multiplies it into dlogits
        gs = grad.detach().to(torch.float32).reshape(1).contiguous()
        _, dl = engine.ce_loss_bwd(lg, lb, ctx.weight, ctx.opts, acc, grad_scale=gs, want_loss=False)
        return dl, None, None, None


class _CERankLossFn(torch.autograd.Function):
    """The criterion pair followed by cova_page_rank_loss_fwd + cova_page_rank_loss_bwd as one autograd node: the ranking
    term and its gradient are added to the pair's loss and dlogits (gradient with respect to the logits only)."""

    @staticmethod
    def forward(ctx, logits, labels, rank_labels, page_start, weight, opts, rank_opts, rank_weight):
        lg, lb, rl, ps = _f32c(logits), _i64c(labels), _i64c(rank_labels), _i64c(page_start)
        acc, _ = engine.ce_loss_fwd(lg, lb, weight, opts, want_pred=False)
        loss, _ = engine.ce_loss_bwd(lg, lb, weight, opts, acc, want_grad=False)
        lists, racc = engine.page_rank_loss_fwd(lg, rl, ps, weight, rank_opts)
        engine.page_rank_loss_bwd(lg, rl, ps, weight, rank_opts, lists, racc, rank_weight, into=(loss, None))
        ctx.save_for_backward(lg, lb, rl, ps, acc, lists, racc)
        ctx.weight, ctx.opts, ctx.rank_opts, ctx.rank_weight = weight, opts, rank_opts, rank_weight
        return loss[0]

    @staticmethod
    def backward(ctx, grad):
        lg, lb, rl, ps, acc, lists, racc = ctx.saved_tensors
        gs = grad.detach().to(torch.float32).reshape(1).contiguous()      # stays on the device, as in _CELossFn
        _, dl = engine.ce_loss_bwd(lg, lb, ctx.weight, ctx.opts, acc, grad_scale=gs, want_loss=False)
        engine.page_rank_loss_bwd(lg, rl, ps, ctx.weight, ctx.rank_opts, lists, racc, ctx.rank_weight, grad_scale=gs,
                                  into=(None, dl))
        return dl, None, None, None, None, None, None, None


class CrossEntropyLoss(nn.Module):
    """torch.nn.CrossEntropyLoss's arguments and defaults on the HIP criterion kernels, plus ``focal_gamma`` (0, or >= 1:
    w[y] (1-p_y)^gamma (-log p_y); not together with label_smoothing).  ``forward(logits [N, C] f32, labels [N] int64)``
    returns the device scalar.  Differences from torch: reduction "none" and probability targets are
    not implemented; "mean" over a zero denominator (every box ignored) gives 0 with a zero gradient, not NaN; a label
    outside [0, C) that is not ``ignore_index`` is skipped like an ignored one instead of raising a device assert.

    ``hard_negative_ratio`` (None: off) and ``hard_negative_min`` add per-page hard-negative mining:
    ``forward(logits, labels, page_start)`` with the pages' row offsets (device int64 [B + 1]) first relabels, without
    gradient, every background row (label 0) outside its page's max(hard_negative_min, floor(ratio * positives)) hardest
    as ``ignore_index`` (one cova_hard_negative_select launch) and scores the rest.

    ``page_rank_weight`` (0: off) adds ``page_rank_weight * R``, the per-page listwise ranking loss of the labelled rows
    among the rows of their page ("Page ranking loss"), with the module's ``weight``, ``ignore_index``
    and ``reduction``; ``forward(logits, labels, page_start)`` is then one autograd node over cova_ce_loss_fwd / _bwd and
    cova_page_rank_loss_fwd / _bwd.  The lists are read from the given labels, whatever mining relabels."""

    def __init__(self, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0, focal_gamma=0.0,
                 hard_negative_ratio=None, hard_negative_min=0, page_rank_weight=0.0):
        super().__init__()
        if reduction == "none":
            raise ValueError('reduction="none" (per-box losses) is not implemented; use "mean" or "sum"')
        w = None if weight is None else torch.as_tensor(weight).detach().to(torch.float32).contiguous().clone()
        if w is not None and w.dim() != 1:
            raise ValueError("weight must be one-dimensional (one value per class), got shape %s" % (tuple(w.shape),))
        # the class count is the logits' width, known at the first forward: until then the weight's own length (the
        # checks of its values and of the scalar options do not depend on it)
        engine.check_loss_options(LOSS_MAX_CLASSES if w is None else max(int(w.numel()), 1), w, label_smoothing,
                                  focal_gamma, None, reduction)
        self.register_buffer("weight", w)
        ig = int(ignore_index)
        self.ignore_index, self.reduction = ig, reduction
        self.label_smoothing, self.focal_gamma = float(label_smoothing), float(focal_gamma)
        self.hard_negative_ratio, self.hard_negative_min = engine.check_mining_options(hard_negative_ratio,
                                                                                       hard_negative_min)
        self.page_rank_weight = engine.check_rank_options(page_rank_weight)

    def forward(self, input, target, page_start=None):
        if self.page_rank_weight != 0.0 and page_start is None:
            raise ValueError("CrossEntropyLoss(page_rank_weight=...) needs page_start (the pages' row offsets, "
                             "int64 [B + 1]) as the third argument of forward")
        if self.hard_negative_ratio is not None and page_start is None:
            raise ValueError("CrossEntropyLoss(hard_negative_ratio=...) needs page_start (the pages' row offsets, "
                             "int64 [B + 1]) as the third argument of forward")
        _require_cuda(input, target)
        if input.dim() != 2 or target.dim() != 1 or target.shape[0] != input.shape[0]:
            raise ValueError("CrossEntropyLoss takes logits [N, C] and class labels [N], got %s and %s"
                             % (tuple(input.shape), tuple(target.shape)))
        if target.is_floating_point():
            raise ValueError("probability targets are not implemented: labels must be integer class indices")
        if self.weight is not None:
            _require_cuda(self.weight)
        opts = engine.check_loss_options(input.shape[1], self.weight, self.label_smoothing, self.focal_gamma,
                                         None, self.reduction)
        # torch's ignore_index may name a class (rows of that class are then skipped): no range check here
        opts["ignore_index"] = self.ignore_index
        given = target
        if self.hard_negative_ratio is not None:
            _require_cuda(page_start)
            with torch.no_grad():
                target, _, _ = engine.hard_negative_select(_f32c(input.detach()), _i64c(target), _i64c(page_start),
                                                           self.hard_negative_ratio, self.hard_negative_min,
                                                           self.ignore_index)
        if self.page_rank_weight != 0.0:
            _require_cuda(page_start)
            if page_start.dim() != 1 or page_start.shape[0] < 2 or page_start.is_floating_point():
                raise ValueError("page_start must hold B + 1 integer row offsets, B >= 1, got shape %s"
                                 % (tuple(page_start.shape),))
            rank_opts = dict(ignore_index=self.ignore_index, reduction=self.reduction)
            return _CERankLossFn.apply(input, target, given, page_start, self.weight, opts, rank_opts,
                                       self.page_rank_weight)
        return _CELossFn.apply(input, target, self.weight, opts)

    def extra_repr(self):
        s = "ignore_index=%d, reduction=%r, label_smoothing=%g, focal_gamma=%g" % (
            self.ignore_index, self.reduction, self.label_smoothing, self.focal_gamma)
        if self.hard_negative_ratio is not None:
            s += ", hard_negative_ratio=%g, hard_negative_min=%d" % (self.hard_negative_ratio, self.hard_negative_min)
        if self.page_rank_weight != 0.0:
            s += ", page_rank_weight=%g" % self.page_rank_weight
        return s
