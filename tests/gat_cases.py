"""The GATv2 kernel cases and what the suites of the graph attention head share (tests/test_gatv2_gpu.py,
tests/test_attn_dropout_gpu.py, the page-layer suites): shapes, hard neighbour tables, boxes, the float64 reference of a
case (tests/gatv2_oracle.py under autograd), the kernels' own gate decisions and the parameter-gradient check."""
import functools

import numpy as np
import torch

from cova_web_object_detection_amd import engine
from helpers import relerr
import edge_oracle as EO
import gatv2_oracle as G2

EDGE_W = np.asarray([1.5, -2.0, 0.75, -0.5, 3.0, -1.25, 2.0, 0.6], np.float32)
ZERO_ROW, DUP_NBR = 7, 9                                  # node 7 names node 9 twice, on channels where z is +0.0 / -0.0

#        N    K    D  pad   (pad: extra floats per row of Wh / h' / g / dWh; odd = unaligned rows = the scalar form)
SHAPES = {"one": (1, 1, 6, 0),              # a single self-loop; fewer channels than lanes, scalar form
          "scalar": (37, 24, 6, 3),         # D % 4 != 0
          "passes": (37, 65, 64, 4),        # K > 64: two lane passes; float4 form, one chunk
          "unaligned": (37, 24, 64, 1),     # D % 4 == 0 but odd leading dimensions: the scalar form at 64 channels
          "wide": (130, 24, 384, 8),        # the second 256-channel chunk part-filled; a hub of in-degree 129
          "general": (130, 100, 96, 4)}     # K = 100, 24 float4 lanes of 64


def random_boxes(rs, n, size):
    """[n, 5] boxes of one page: some overlap, some lie apart (every edge feature takes values off zero)."""
    wh = rs.uniform(4, 0.25 * size, (n, 2))
    xy = rs.uniform(0, 1, (n, 2)) * (size - wh)
    return np.concatenate([np.zeros((n, 1)), xy, xy + wh], 1).astype(np.float32)


def make_table(rs, N, K, out_of_range=True):
    """Arbitrary ids with: an all-pad row (3), a row with one valid slot (4), ids >= N, self-loops, one neighbour named
    twice in a row, a node nobody names (N - 1) and a hub every other row names (5)."""
    ctx = rs.randint(-1, N, (N, K)).astype(np.int64)
    if N == 1:
        return np.zeros((1, K), np.int64)
    ctx[::5, 0] = np.arange(N)[::5]                           # self-loops
    if K >= 4:
        ctx[:, K - 1] = 5                                     # the hub
        ctx[ZERO_ROW, 1:3] = DUP_NBR                          # the same neighbour twice
        if out_of_range:
            ctx[11, 1], ctx[12, 2] = N, N + 1000
    ctx[3] = -1
    ctx[4] = -1
    ctx[4, K // 2] = 8
    ctx[ctx == N - 1] = -1                                    # in-degree 0
    return ctx


@functools.lru_cache(maxsize=None)
def gat_case(name, out_of_range=True):
    N, K, D, pad = SHAPES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    ctx = make_table(rs, N, K, out_of_range)
    Wh = rs.standard_normal((N, 2 * D)).astype(np.float32)
    if N > DUP_NBR and K >= 4:                                # z exactly +0.0 on channels 0, 1 and -0.0 on channel 2
        Wh[DUP_NBR, D:D + 2] = -Wh[ZERO_ROW, :2]
        Wh[ZERO_ROW, 2] = Wh[DUP_NBR, D + 2] = -0.0
    bb = random_boxes(rs, N, 1280.0)
    aw = (rs.standard_normal(D) / np.sqrt(D)).astype(np.float32)
    aw[:3] = [0.5, -0.5, 0.5]                                 # the channels of the zero sums weigh in the gradient
    case = dict(name=name, N=N, K=K, D=D, pad=pad, ctx=ctx, Wh=Wh, phi=EO.edge_features(bb, ctx, 1280.0, 1280.0),
                aw=aw, ab=rs.standard_normal(1).astype(np.float32), g=rs.standard_normal((N, D)).astype(np.float32))
    case["ref"] = oracle64(case, None)
    case["ref_edge"] = oracle64(case, EDGE_W)
    return case


def oracle64(case, edge_w, gate=None, slope=0.2):
    D = case["D"]
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    Wh = f64(case["Wh"]).requires_grad_(True)
    aw, ab = f64(case["aw"]).requires_grad_(True), f64(case["ab"]).requires_grad_(True)
    ew = None if edge_w is None else f64(edge_w).view(1, 8).requires_grad_(True)
    hp, attn = G2.attend(Wh[:, :D], Wh[:, D:], torch.from_numpy(case["ctx"]), aw, ab, slope, ew,
                         None if edge_w is None else f64(case["phi"]), gate)
    (hp * f64(case["g"])).sum().backward()
    return dict(hp=hp.detach().numpy(), attn=attn.detach().numpy(), dWh=Wh.grad.numpy(), daw=aw.grad.numpy(),
                dab=ab.grad.numpy(), dew=None if ew is None else ew.grad.numpy().reshape(-1))


def device_gates(Wh, ctx):
    """(Wh_i + Wh_j[ctx]) > 0 in float32 from a GATv2 head's saved Wh [N, 2D]: the kernels' own decisions."""
    N, D = Wh.shape[0], Wh.shape[1] // 2
    ok = (ctx >= 0) & (ctx < N)
    rows = torch.cat((Wh[:, D:], Wh.new_zeros(1, D)))
    return ((Wh[:, :D].unsqueeze(1) + rows[torch.where(ok, ctx, torch.full_like(ctx, N))]) > 0).cpu()


def recorded_heads(monkeypatch):
    """Every engine.gat_fwd call's saved dict, in call order (layer-major, heads ascending)."""
    svs, real = [], engine.gat_fwd

    def fn(*a, **kw):
        sv = real(*a, **kw)
        svs.append(sv)
        return sv
    monkeypatch.setattr(engine, "gat_fwd", fn)
    return svs


def check_param_grads(module, sd):
    """Every parameter gradient to 1e-4; a v2 ``attention_layer.bias`` shifts all scores of a row alike, so its gradient
    is analytically zero (round-off in both implementations) and is held on the scale of its head's attention weight."""
    for key, p in module.named_parameters():
        ref = sd["gat." + key].grad
        scale = None
        if key.endswith("attention_layer.bias"):
            scale = float(sd["gat." + key[:-len("bias")] + "weight"].grad.abs().max())
            assert scale > 0
        assert relerr(p.grad.cpu(), ref, scale) < 1e-4, key
