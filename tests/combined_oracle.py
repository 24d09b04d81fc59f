"""CPU restatement of the WHOLE context head with any subset of its opt-in layers on: one composition of the per-feature
oracles (edge_oracle, gatv2_oracle, attn_dropout_oracle, readout_oracle, page_attn_oracle, page_attn_geo_oracle), which it
imports and does not restate.  The columns behind the own features are, in the decoder's order,

    [ GAT stack D | page readout G | page attention E ]          (each part present only when its weights are in ``sd``)

* GAT stack: oracle.cova_oracle.gat_stack's layering (heads side by side, layers chained); every head is the static oracle,
  the edge-aware one (``edge_layer.weight``), the GATv2 one (``attention_layer.weight`` [1, D]) or, with a keep mask for its
  prefix, attn_dropout_oracle.head.  Forced LeakyReLU gates: ``routing["gate_" + prefix + "leaky"]`` ([N, K], GATv2 [N, K, D]).
* page readout (``page_readout.W.weight``): readout_oracle.readout of the OWN features; gates
  ``routing["gate_page_readout.leaky"]``.
* page attention (``page_attention.qkv.weight``): page_attn_oracle.page_attention of the OWN features, or page_attn_geo_oracle's
  with ``page_attention.geometry.weight``.

Which options are on is read off the state dict, so one function states every model.  A state dict without attention heads
(``use_context=False``) gives [r | O]: O.forward reaches its gat_stack hook under ``use_context=True`` only, so such a model
is stated to it with that flag set and the columns come out as [own | r | O], the no-context head.

It runs in the dtype of its inputs (float64 for the kernel tests) under autograd.  ``patched(...)`` returns the replacements
for BOTH oracle.cova_oracle.gat and oracle.cova_oracle.gat_stack of one batch; ``on_table(visual)`` the replacements for
convnet and roi_pool that hand O.forward a given table of visual features (the cached-feature path: the head alone);
``roi_pool_in_dtype`` a replacement for roi_pool that lets O.forward run the WHOLE model in float64."""
import torch

from oracle import cova_oracle as O
import attn_dropout_oracle as AD
import edge_oracle as EO
import gatv2_oracle as G2
import page_attn_geo_oracle as PG
import page_attn_oracle as PA
import readout_oracle as RO

_PLAIN_GAT = O.gat                       # taken at import: a test may have replaced O.gat by the time patched() runs
RO_KEY, RO_GATE = RO.PREFIX + "W.weight", "gate_" + RO.PREFIX + "leaky"
EDGE, GEO_KEY = "edge_layer.weight", PG.GEO_KEY


class Batch:
    """What the options read of a batch besides the neighbour table: ``page_start`` (B + 1 row offsets; readout and page
    attention), ``bboxes`` [N, 5] and ``page_size`` = (height, width) (edge term and geometry bias), ``heads`` of the page
    attention, ``keeps`` {head prefix: bool [N, K]} with the rate ``attention_dropout`` (absent prefix: no dropout)."""

    def __init__(self, page_start=None, bboxes=None, page_size=None, heads=1, keeps=None, attention_dropout=0.0):
        self.page_start = None if page_start is None else [int(v) for v in page_start]
        self.bboxes, self.page_size, self.heads = bboxes, page_size, int(heads)
        self.keeps, self.p = dict(keeps or {}), float(attention_dropout)
        self._phi, self._page_phi = {}, None

    def phi(self, context_indices, dtype):
        """edge features of the neighbour table, float32 values (the device's bits) in ``dtype``"""
        key = (context_indices.data_ptr(), tuple(context_indices.shape))
        if key not in self._phi:
            self._phi[key] = torch.from_numpy(EO.edge_features(self.bboxes.detach().numpy(), context_indices.numpy(),
                                                               self.page_size[1], self.page_size[0]))
        return self._phi[key].to(dtype)

    def page_phi(self):
        if self._page_phi is None:
            self._page_phi = PG.page_features(self.bboxes.detach().numpy(), self.page_start, self.page_size[1],
                                              self.page_size[0])
        return self._page_phi


def gat_head(batch, h, context_indices, sd, alpha=0.2, prefix="gat.", routing=None):
    """One attention head with whatever options its entries and the batch switch on -> (h' [N, D], attn [N, K] before
    dropout).  Without a keep mask it IS the sibling oracle of that head (the same function, the same bits)."""
    phi = batch.phi(context_indices, h.dtype) if prefix + EDGE in sd else None
    v2 = G2.is_v2(sd, prefix)
    gate = routing.get("gate_" + prefix + "leaky") if routing else None
    keep = batch.keeps.get(prefix)
    if keep is not None:
        return AD.head("gatv2" if v2 else "gat", h, context_indices, sd, prefix, keep, batch.p, phi, gate, alpha)
    if v2:
        return G2.gat_v2(h, context_indices, sd, phi, alpha, True, prefix, gate)
    if phi is not None:
        return EO.gat(h, context_indices, sd, phi, alpha, True, prefix, routing)
    return _PLAIN_GAT(h, context_indices, sd, alpha, True, prefix, routing)


def head(batch, h_i, context_indices, sd, alpha=0.2, routing=None, return_all=False):
    """oracle.cova_oracle.gat_stack's signature behind ``batch`` -> (columns [N, D + G + E], attention of the LAST layer's
    first head).  ``return_all``: also {"attn": {prefix: [N, K]}, "readout": (beta, r, u, P), "page_attn": (A, lse, qkv)}."""
    parts, attn0, inter = [], h_i[:, :0].detach(), {"attn": {}}
    h = h_i
    for heads in O.gat_prefixes(sd):
        outs = []
        for p in heads:
            o, a = gat_head(batch, h, context_indices, sd, alpha, p, routing)
            outs.append(o)
            inter["attn"][p] = a
            if p == heads[0]:
                attn0 = a
        h = torch.cat(outs, dim=1)
    if O.gat_prefixes(sd):
        parts.append(h)
    if RO_KEY in sd:
        rows, beta, r, u, P = RO.readout(h_i, sd, batch.page_start, alpha, routing.get(RO_GATE) if routing else None,
                                         return_all=True)
        parts.append(rows)
        inter["readout"] = (beta, r, u, P)
    if PA.KEY in sd:
        if GEO_KEY in sd:
            out, A, lse, qkv = PG.page_attention(h_i, sd, batch.page_start, batch.heads, batch.page_phi(), return_all=True)
        else:
            out, A, lse, qkv = PA.page_attention(h_i, sd, batch.page_start, batch.heads, return_all=True)
        parts.append(out)
        inter["page_attn"] = (A, lse, qkv)
    cols = torch.cat(parts, dim=1) if parts else h_i[:, :0]
    return (cols, attn0, inter) if return_all else (cols, attn0)


def patched(page_start=None, bboxes=None, page_size=None, heads=1, keeps=None, attention_dropout=0.0, tap=None):
    """-> (gat, gat_stack): the replacements for oracle.cova_oracle.gat and oracle.cova_oracle.gat_stack (monkeypatch both)
    that make O.forward / O.loss_and_grads state the whole model of this batch with any subset of the options; the decoder
    reads its width from the state dict.  ``tap`` (a dict): receives the intermediates of the last call (head's
    ``return_all``)."""
    batch = Batch(page_start, bboxes, page_size, heads, keeps, attention_dropout)

    def gat(h_i, context_indices, sd, alpha=0.2, return_attn_wts=False, prefix="gat.", routing=None):
        o, a = gat_head(batch, h_i, context_indices, sd, alpha, prefix, routing)
        return (o, a) if return_attn_wts else o

    def gat_stack(h_i, context_indices, sd, alpha=0.2, routing=None):
        cols, attn0, inter = head(batch, h_i, context_indices, sd, alpha, routing, return_all=True)
        if tap is not None:
            tap.clear()
            tap.update(inter)
        return cols, attn0
    return gat, gat_stack


def on_table(visual):
    """-> (convnet, roi_pool): replacements for oracle.cova_oracle.convnet and oracle.cova_oracle.roi_pool that hand
    O.forward the rows of ``visual`` [N, n_vis] as the visual columns (any dtype): everything in front of the head is given,
    O.forward states the head alone.  ``images`` is then read for its height only."""
    def convnet(images, sd, training, routing=None):
        return images

    def roi_pool(feat, rois, output_size, spatial_scale, forced_argmax=None):
        return visual
    return convnet, roi_pool


def roi_pool_in_dtype(feat, rois, output_size, spatial_scale, forced_argmax=None):
    """oracle.cova_oracle.roi_pool for a feature map of any dtype (the C restatement is float32): the values of ``feat`` at
    the arg-max positions, gathered in feat's dtype, so that autograd routes the gradient there.  The positions are the
    forced ones (the implementation under test's, [N, C*PH*PW] flat h*W+w, -1 = empty bin) or else the C restatement's on
    the float32 copy of ``feat``; a forced position that is not the maximum is within round-off of it (tests/helpers.py,
    assert_routing_near_ties)."""
    n, C = rois.shape[0], feat.shape[1]
    if forced_argmax is None:
        _, arg = O.roi_pool_argmax(feat.detach(), rois, output_size, spatial_scale)
    else:
        arg = forced_argmax.reshape(n, C, int(output_size[0]), int(output_size[1]))
    arg = arg.long()
    bidx = rois[:, 0].long().view(-1, 1, 1, 1).expand_as(arg)
    cidx = torch.arange(C).view(1, -1, 1, 1).expand_as(arg)
    return feat.flatten(2)[bidx, cidx, arg.clamp(min=0)] * (arg >= 0)
