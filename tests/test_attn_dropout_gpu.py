"""GPU tests of the attention dropout: cova_gat_fwd_drop / cova_gat_bwd_drop / cova_gat2_fwd_drop / cova_gat2_bwd_drop
through the C ABI on framed, NaN-padded buffers against the float64 torch oracle (tests/attn_dropout_oracle.py: the mask
from the numpy restatement of the counter hash, autograd's backward), then engine.gat_fwd, the modules under autograd, and
CoVA / HotPathTrainer with the option on.

Bounds: those of tests/test_gatv2_gpu.py -- max-abs error over max-abs reference below 1e-5 for h' and attn, below 1e-4 for
dWh, d_att_w and d_edge_w; d_att_b on the d_att_w scale.  A wrong mask bit moves h' by O(alpha * |Wh|), four orders above
the bound, so the forward comparison pins the mask, its index and its stream.  The static oracle takes its LeakyReLU
branches from its own float64 pre-activations; the cases are asserted to have no valid slot within 1e-5 of zero, where the
kernel's f32 sum could decide otherwise.  The GATv2 gates are sums of two f32 numbers: their sign is exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import CoVA, GraphAttentionLayer, MultiHeadGraphAttention  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset, attention_rows  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import compare_grads, DEV, framed, GRAD_TOL, GUARD, load_case, NAN, padded, profiled, relerr, survived  # noqa: E402
import attn_dropout_oracle as AD  # noqa: E402
import edge_oracle as EO  # noqa: E402
import gat_cases as GC  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from gat_cases import EDGE_W  # noqa: E402
from trainer_cases import page_set, seeded  # noqa: E402

RATES = (0.5, 0.6)
SEED = engine.attention_dropout_seed(engine.dropout_base(123, 1), 0, 0)

#                  N    K    D  pad
STATIC_SHAPES = {"one": (1, 1, 6, 0),              # a single self-loop
                 "partial": (37, 24, 6, 3),        # wide form, one partial 64-channel chunk
                 "wide6": (130, 24, 384, 8),       # wide form, ND = 6; a hub of in-degree 129
                 "beyond": (37, 24, 520, 0),       # D beyond the wide forms (9 chunks): the general kernels, one lane pass
                 "passes": (37, 65, 64, 4),        # K > 64: two lane passes
                 "general": (130, 100, 96, 1)}
CASES = [("gat", n) for n in STATIC_SHAPES] + [("gatv2", n) for n in GC.SHAPES]
IDS = ["%s-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def gat_case(mode, name):
    """operands of one case (host arrays); the GATv2 ones are tests/gat_cases.py's"""
    if mode == "gatv2":
        return dict(GC.gat_case(name), mode=mode)
    N, K, D, pad = STATIC_SHAPES[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 1)
    ctx = GC.make_table(rs, N, K)
    bb = GC.random_boxes(rs, N, 1280.0)
    return dict(mode=mode, name=name, N=N, K=K, D=D, pad=pad, ctx=ctx, Wh=rs.standard_normal((N, 2 * D)).astype(np.float32),
                phi=EO.edge_features(bb, ctx, 1280.0, 1280.0), aw=(rs.standard_normal(2 * D) / np.sqrt(D)).astype(np.float32),
                ab=rs.standard_normal(1).astype(np.float32), g=rs.standard_normal((N, D)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def oracle64(mode, name, edge, p=0.0, seed=None):
    """float64 forward and autograd backward of a case with the numpy mask of (p, seed); seed None: no dropout"""
    case = gat_case(mode, name)
    N, K, D = case["N"], case["K"], case["D"]
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    Wh = f64(case["Wh"]).requires_grad_(True)
    aw, ab = f64(case["aw"]).requires_grad_(True), f64(case["ab"]).requires_grad_(True)
    ew = f64(EDGE_W).view(1, 8).requires_grad_(True) if edge else None
    keep = None if seed is None else AD.keep_mask(p, seed, N, K)
    hp, attn, u = AD.attend(mode, Wh[:, :D], Wh[:, D:], torch.from_numpy(case["ctx"]), aw, ab, keep, p, 0.2, ew,
                            f64(case["phi"]) if edge else None)
    if u is not None:                                         # no LeakyReLU decision of the static score near its kink
        ok = (case["ctx"] >= 0) & (case["ctx"] < N)
        assert float(u.detach().abs().numpy()[ok].min()) > 1e-5, (mode, name, edge)
    (hp * f64(case["g"])).sum().backward()
    return dict(hp=hp.detach().numpy(), attn=attn.detach().numpy(), dWh=Wh.grad.numpy(), daw=aw.grad.numpy(),
                dab=ab.grad.numpy(), dew=None if ew is None else ew.grad.numpy().reshape(-1), keep=keep)


def launch(case, edge=False, drop=None, edge_w=EDGE_W):
    """forward + backward of one mode on framed buffers -> host arrays (guards checked).  ``drop`` = (p, seed): the _drop
    entry points; None: the entry points that exist without the option."""
    mode, N, K, D, pad = case["mode"], case["N"], case["K"], case["D"], case["pad"]
    v2 = mode == "gatv2"
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    Wh, g = padded(case["Wh"], 2 * D + pad), padded(case["g"], D + pad)
    aw, ab, ctx = dev(case["aw"]), dev(case["ab"]), dev(case["ctx"])
    phi = ew = dew = dew_buf = ws = None
    if edge:
        phi, ew = dev(case["phi"]), dev(np.asarray(edge_w, np.float32))
        dew_buf, dew = framed(1, 8, 8)
    W = D if v2 else 2 * D
    attn_b, attn = framed(N, K, K)
    hp_b, hp = framed(N, D, D + pad)
    du_b, du = framed(N, K, K)
    dWh_b, dWh = framed(N, 2 * D, 2 * D + pad)
    daw_b, daw = framed(1, W, W)
    dab_b, dab = framed(1, 1, 1)
    st_b, st = framed(4, N, N)                                # rows: s, t, ds, dt of the static mode
    csr = torch.zeros((engine.query("cova_gat_transpose_ints", N, K),), dtype=torch.int32, device=DEV)
    engine.call("cova_gat_transpose", ctx, N, K, csr)
    nws = engine.query("cova_gat2_workspace_floats", N, K, D) if v2 else (
        engine.query("cova_gat_edge_workspace_floats", N, K) if edge else 0)
    if nws:
        ws = torch.full((nws + 16,), NAN, device=DEV)
        ws[nws:] = GUARD
    lw, lh, lg = 2 * D + pad, D + pad, D + pad
    if v2:
        if drop is None:
            engine.call("cova_gat2_fwd", Wh, lw, aw, ab, ctx, phi, ew, N, K, D, 0.2, attn, hp, lh)
            engine.call("cova_gat2_bwd", g, lg, Wh, lw, attn, ctx, aw, phi, ew, N, K, D, 0.2, dWh, lw, daw, dab, dew, csr, du, ws)
        else:
            engine.call("cova_gat2_fwd_drop", Wh, lw, aw, ab, ctx, phi, ew, N, K, D, 0.2, drop[0], drop[1], attn, hp, lh)
            engine.call("cova_gat2_bwd_drop", g, lg, Wh, lw, attn, ctx, aw, phi, ew, N, K, D, 0.2, drop[0], drop[1], dWh, lw,
                        daw, dab, dew, csr, du, ws)
    elif drop is not None:
        engine.call("cova_gat_fwd_drop", Wh, lw, aw, ab, ctx, phi, ew, N, K, D, 0.2, drop[0], drop[1], st[0], st[1], attn, hp, lh)
        engine.call("cova_gat_bwd_drop", g, lg, Wh, lw, st[0], st[1], attn, ctx, aw, phi, ew, N, K, D, 0.2, drop[0], drop[1],
                    dWh, lw, st[2], st[3], daw, dab, dew, csr, du, ws)
    elif edge:
        engine.call("cova_gat_fwd_edge", Wh, lw, aw, ab, ctx, phi, ew, N, K, D, 0.2, st[0], st[1], attn, hp, lh)
        engine.call("cova_gat_bwd_edge", g, lg, Wh, lw, st[0], st[1], attn, ctx, aw, phi, ew, N, K, D, 0.2, dWh, lw, st[2],
                    st[3], daw, dab, dew, csr, du, ws)
    else:
        engine.call("cova_gat_fwd", Wh, lw, aw, ab, ctx, N, K, D, 0.2, st[0], st[1], attn, hp, lh)
        engine.call("cova_gat_bwd", g, lg, Wh, lw, st[0], st[1], attn, ctx, aw, N, K, D, 0.2, dWh, lw, st[2], st[3], daw, dab,
                    csr, du)
    torch.cuda.synchronize()
    if nws:
        assert (ws[nws:] == GUARD).all()
    out = dict(attn=survived(attn_b, N, K), hp=survived(hp_b, N, D), du=survived(du_b, N, K),
               dWh=survived(dWh_b, N, 2 * D), daw=survived(daw_b, 1, W).reshape(-1), dab=survived(dab_b, 1, 1).reshape(-1))
    if not v2:
        out["st"] = survived(st_b, 4, N)
    if edge:
        out["dew"] = survived(dew_buf, 1, 8).reshape(-1)
    return out


def check_against(got, ref, what):
    errs = {k: relerr(got[k], ref[k]) for k in ("hp", "attn", "dWh", "daw")}
    errs["dab"] = relerr(got["dab"], ref["dab"], scale=np.abs(ref["daw"]).max())
    if ref.get("dew") is not None:
        errs["dew"] = relerr(got["dew"], ref["dew"])
    print(what, {k: "%.2e" % v for k, v in errs.items()})
    for k, e in errs.items():
        assert e < (1e-5 if k in ("hp", "attn") else 1e-4), (what, k, e)


def same_bits(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ---------------------------------------------------------------- 1. the kernels through the C ABI
@pytest.mark.parametrize("mode,name", CASES, ids=IDS)
def test_forward_and_backward_match_the_float64_oracle_and_attn_is_undropped(mode, name):
    case = gat_case(mode, name)
    N, K, D = case["N"], case["K"], case["D"]
    for edge in (False, True):
        plain = launch(case, edge)
        for p in RATES:
            got, ref = launch(case, edge, (p, SEED)), oracle64(mode, name, edge, p, SEED)
            check_against(got, ref, "%s %s p=%.1f%s" % (mode, name, p, " + edge" if edge else ""))
            same_bits(got, plain, ("attn",))                  # the distribution before dropout, bit for bit
            if not mode == "gatv2":
                assert np.array_equal(got["st"][:2].view(np.uint32), plain["st"][:2].view(np.uint32))        # s, t
            keep, pads = ref["keep"], (case["ctx"] < 0) | (case["ctx"] >= N)
            assert not got["du"][pads].any()
            if N > 1:
                assert 0.2 < 1.0 - keep.mean() < 0.8 and relerr(got["hp"], plain["hp"]) > 1e-2     # the option is live
                assert not got["hp"][3].any() and not got["dWh"][N - 1, D:].any()    # all-pad row; in-degree 0
                # a dropped valid slot still has a gradient through the softmax
                dropped = ~keep & ~pads
                assert np.abs(got["du"][dropped]).max() > 0
                live = ~pads.all(1)
                assert np.allclose(got["attn"][live].sum(1), 1.0, atol=1e-5)
            else:                                             # K = 1: the self-loop weighs inv, or the row is dropped
                want = np.float32(AD.inv_keep(p)) * case["Wh"][0, D:] if keep[0, 0] else np.zeros(D, np.float32)
                assert got["attn"][0, 0] == 1.0 and np.array_equal(got["hp"][0], want)


@pytest.mark.parametrize("mode", ["gat", "gatv2"])
def test_a_row_whose_valid_slots_are_all_dropped_is_exactly_zero_and_passes_no_gradient(mode):
    """N 37, K 5 at p = 0.6: the seed is searched with the numpy hash for a row of >= 3 valid slots that are all dropped"""
    N, K, D = 37, 5, 64
    rs = np.random.RandomState(31)
    ctx = GC.make_table(rs, N, K)
    valid = (ctx >= 0) & (ctx < N)
    case = dict(mode=mode, name="dropped", N=N, K=K, D=D, pad=4, ctx=ctx, Wh=rs.standard_normal((N, 2 * D)).astype(np.float32),
                phi=None, aw=(rs.standard_normal(D if mode == "gatv2" else 2 * D) / 8).astype(np.float32),
                ab=rs.standard_normal(1).astype(np.float32), g=rs.standard_normal((N, D)).astype(np.float32))
    seed = row = None
    for cand in range(SEED, SEED + 200):
        keep = AD.keep_mask(0.6, cand, N, K)
        rows = np.nonzero((valid.sum(1) >= 3) & ~(keep & valid).any(1))[0]
        if rows.size:
            seed, row = cand, int(rows[0])
            break
    assert seed is not None
    got, plain = launch(case, False, (0.6, seed)), launch(case, False)
    assert not got["hp"][row].any() and plain["hp"][row].any()
    assert not got["du"][row].any() and plain["du"][row].any()
    assert all(np.isfinite(v).all() for v in got.values())
    same_bits(got, plain, ("attn",))
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    Wh, aw, ab = f64(case["Wh"]).requires_grad_(True), f64(case["aw"]).requires_grad_(True), f64(case["ab"]).requires_grad_(True)
    hp, attn, _ = AD.attend(mode, Wh[:, :D], Wh[:, D:], torch.from_numpy(ctx), aw, ab, keep, 0.6)
    (hp * f64(case["g"])).sum().backward()
    check_against(got, dict(hp=hp.detach().numpy(), attn=attn.detach().numpy(), dWh=Wh.grad.numpy(), daw=aw.grad.numpy(),
                            dab=ab.grad.numpy()), mode + " all-dropped row")


@pytest.mark.parametrize("mode,name", [("gat", "partial"), ("gat", "wide6"), ("gat", "beyond"), ("gat", "general"),
                                       ("gatv2", "scalar"), ("gatv2", "wide"), ("gatv2", "general")])
def test_one_seed_gives_the_same_bits_twice_and_another_seed_another_mask(mode, name):
    case = gat_case(mode, name)
    for edge in (False, True):
        a, b = launch(case, edge, (0.5, SEED)), launch(case, edge, (0.5, SEED))
        same_bits(a, b)
        c = launch(case, edge, (0.5, SEED + 1))
        same_bits(a, c, ("attn",))
        assert relerr(c["hp"], a["hp"]) > 1e-2 and relerr(c["dWh"], a["dWh"]) > 1e-2
    # p = 0 through the _drop entry points keeps every slot at weight attn * 1: the plain entry points' bits
    same_bits(launch(case, False, (0.0, SEED)), launch(case, False))


@pytest.mark.parametrize("mode", ["gat", "gatv2"])
def test_entry_points_refuse_bad_rates_sizes_and_mismatched_groups(mode):
    N, K, D = 8, 6, 16
    v2 = mode == "gatv2"
    z = lambda *shape: torch.zeros(shape, device=DEV)
    ctx = torch.zeros((N, K), dtype=torch.int64, device=DEV)
    hp, attn = torch.full((N, D), GUARD, device=DEV), torch.full((N, K), GUARD, device=DEV)
    dWh = torch.full((N, 2 * D), GUARD, device=DEV)
    Wh, aw, ab, phi, ew, dew = z(N, 2 * D), z(D if v2 else 2 * D), z(1), z(N, K, 8), z(8), z(8)
    g, du, daw, dab, s, t, ds, dt = z(N, D), z(N, K), z(D if v2 else 2 * D), z(1), z(N), z(N), z(N), z(N)
    csr = torch.zeros((engine.query("cova_gat_transpose_ints", N, K),), dtype=torch.int32, device=DEV)
    engine.call("cova_gat_transpose", ctx, N, K, csr)
    ews = z(max(engine.query("cova_gat_edge_workspace_floats", N, K), 1))
    if v2:
        ws = z(engine.query("cova_gat2_workspace_floats", N, K, D))
        fwd, good_f = "cova_gat2_fwd_drop", [Wh, 2 * D, aw, ab, ctx, None, None, N, K, D, 0.2, 0.5, 7, attn, hp, D]
        bwd, good_b = "cova_gat2_bwd_drop", [g, D, Wh, 2 * D, attn, ctx, aw, None, None, N, K, D, 0.2, 0.5, 7, dWh, 2 * D, daw,
                                             dab, None, csr, du, ws]
        f_at, b_at = dict(p=11, K=8, phi=5, ew=6), dict(p=13, K=10, phi=7, ew=8, dew=19, ws=None)
    else:
        fwd, good_f = "cova_gat_fwd_drop", [Wh, 2 * D, aw, ab, ctx, None, None, N, K, D, 0.2, 0.5, 7, s, t, attn, hp, D]
        bwd, good_b = "cova_gat_bwd_drop", [g, D, Wh, 2 * D, s, t, attn, ctx, aw, None, None, N, K, D, 0.2, 0.5, 7, dWh, 2 * D,
                                            ds, dt, daw, dab, None, csr, du, None]
        f_at, b_at = dict(p=11, K=8, phi=5, ew=6), dict(p=15, K=12, phi=9, ew=10, dew=23, ws=26)

    def bad(args, changes):
        a = list(args)
        for i, v in changes.items():
            a[i] = v
        return a
    f_bad = [{f_at["p"]: v} for v in (-0.25, 1.0, 1.5, NAN, float("inf"))]
    f_bad += [{f_at["K"]: 0}, {f_at["K"]: engine.GAT_MAX_K + 1}, {f_at["phi"]: phi}, {f_at["ew"]: ew},
              {f_at["phi"]: phi.view(-1)[1:], f_at["ew"]: ew}]
    for ch in f_bad:
        with pytest.raises(_lib.CovaHipError):
            engine.call(fwd, *bad(good_f, ch))
    b_bad = [{b_at["p"]: v} for v in (-0.25, 1.0, 1.5, NAN, float("inf"))]
    b_bad += [{b_at["K"]: 0}, {b_at["K"]: engine.GAT_MAX_K + 1}, {b_at["phi"]: phi}, {b_at["ew"]: ew}, {b_at["dew"]: dew},
              {b_at["phi"]: phi, b_at["ew"]: ew}, {b_at["phi"]: phi, b_at["dew"]: dew}]
    if not v2:                                                # the static group has a fourth member, the workspace
        b_bad += [{b_at["ws"]: ews}, {b_at["phi"]: phi, b_at["ew"]: ew, b_at["dew"]: dew}]
    for ch in b_bad:
        with pytest.raises(_lib.CovaHipError):
            engine.call(bwd, *bad(good_b, ch))
    torch.cuda.synchronize()
    assert (hp == GUARD).all() and (attn == GUARD).all() and (dWh == GUARD).all()        # nothing was launched
    # N == 0 where the plain entry points have it
    if v2:
        engine.call(fwd, None, 2 * D, None, None, None, None, None, 0, K, D, 0.2, 0.5, 7, None, None, D)
        engine.call(bwd, None, D, None, 2 * D, None, None, None, None, None, 0, K, D, 0.2, 0.5, 7, None, 2 * D, None, None,
                    None, None, None, None)
    else:
        engine.call(fwd, *bad(good_f, {7: 0}))
        with pytest.raises(_lib.CovaHipError):
            engine.call(bwd, *bad(good_b, {11: 0}))
    torch.cuda.synchronize()
    assert (hp == GUARD).all() and (dWh == GUARD).all()
    engine.call(fwd, *good_f)                                 # and the good calls are good, with and without the group
    engine.call(bwd, *good_b)
    engine.call(fwd, *bad(good_f, {f_at["phi"]: phi, f_at["ew"]: ew}))
    full = {b_at["phi"]: phi, b_at["ew"]: ew, b_at["dew"]: dew}
    if not v2:
        full[b_at["ws"]] = ews
    engine.call(bwd, *bad(good_b, full))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(hp).all()) and (hp != GUARD).all() and bool(torch.isfinite(dWh).all())


# ---------------------------------------------------------------- 2. engine.gat_fwd and the modules
def head_params(rs, Fd, D, mode, edge):
    p = {"gat.W_i.weight": rs.standard_normal((D, Fd)) / np.sqrt(Fd), "gat.W_j.weight": rs.standard_normal((D, Fd)) / np.sqrt(Fd),
         "gat.attention_layer.weight": rs.standard_normal((1, D if mode == "gatv2" else 2 * D)) / np.sqrt(D),
         "gat.attention_layer.bias": rs.standard_normal(1)}
    if edge:
        p["gat.edge_layer.weight"] = EDGE_W.reshape(1, 8)
    return {k: torch.from_numpy(np.asarray(v, np.float32)).to(DEV) for k, v in p.items()}


@pytest.mark.parametrize("mode", ["gat", "gatv2"])
@pytest.mark.parametrize("edge", [False, True])
def test_engine_without_a_rate_is_the_existing_path_bit_for_bit(mode, edge):
    rs = np.random.RandomState(3)
    N, Fd, D, K = 70, 20, 16, 12
    ctx = torch.from_numpy(GC.make_table(rs, N, K)).to(DEV)
    params = head_params(rs, Fd, D, mode, edge)
    phi = torch.from_numpy(EO.edge_features(GC.random_boxes(rs, N, 400.0), ctx.cpu().numpy(), 400, 400)).to(DEV) if edge else None
    h = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32)).to(DEV)
    g = torch.from_numpy(rs.standard_normal((N, D)).astype(np.float32)).to(DEV)

    def run(**kw):
        hp, dh = torch.full((N, D), NAN, device=DEV), torch.full((N, Fd), NAN, device=DEV)
        sv = engine.gat_fwd(h, Fd, N, Fd, ctx, params, hp, D, phi=phi, attention=mode, **kw)
        grads = engine.gat_bwd(sv, g, D, params, dh, Fd, False)
        return dict(grads, hp=hp, dh=dh, attn=sv["attn"]), sv
    (ref, sv0), calls0 = profiled(lambda: run())
    assert sv0["drop"] is None and not any(n.endswith("_drop") for n in calls0)
    for drop in (None, (0.0, 99), (0, 0)):
        (out, sv), calls = profiled(lambda: run(drop=drop))
        assert sv["drop"] is None and calls == calls0
        for k in ref:
            assert torch.equal(out[k], ref[k]), k
    (on, sv), calls = profiled(lambda: run(drop=(0.5, 99)))
    assert sv["drop"] == (0.5, 99)
    fwd, bwd = ("cova_gat2_fwd", "cova_gat2_bwd") if mode == "gatv2" else (
        ("cova_gat_fwd_edge", "cova_gat_bwd_edge") if edge else ("cova_gat_fwd", "cova_gat_bwd"))
    stem = "cova_gat2_" if mode == "gatv2" else "cova_gat_"
    want = {k: v for k, v in calls0.items() if k not in (fwd, bwd)}
    want.update({stem + "fwd_drop": 1, stem + "bwd_drop": 1})
    assert calls == want
    assert torch.equal(on["attn"], ref["attn"]) and not torch.equal(on["hp"], ref["hp"])
    for bad in ((1.0, 1), (-0.1, 1), (NAN, 1)):
        with pytest.raises(ValueError, match="attention_dropout"):
            run(drop=bad)


def static_gates(sv):
    """the LeakyReLU decisions of a static head from its saved s and t (tests/helpers.py, routing_from_saved)"""
    t = torch.cat((sv["t"], sv["t"].new_zeros(1)))
    ctx = sv["ctx"]
    ok = (ctx >= 0) & (ctx < sv["N"])
    return ((sv["s"].view(-1, 1) + t[torch.where(ok, ctx, torch.full_like(ctx, sv["N"]))]) > 0).cpu()


def gates_of(sv):
    return GC.device_gates(sv["Wh"], sv["ctx"]) if sv.get("attention") == "gatv2" else static_gates(sv)


@pytest.mark.parametrize("mode", ["gat", "gatv2"])
def test_layer_under_autograd_matches_the_oracle_in_train_mode_and_is_the_plain_layer_in_eval_mode(monkeypatch, mode):
    rs = np.random.RandomState(13)
    N, Fd, D, K, p, seed = 131, 24, 8, 9, 0.5, 41
    ctx_np = GC.make_table(rs, N, K)
    torch.manual_seed(11)
    layer = GraphAttentionLayer(Fd, D, attention=mode, attention_dropout=p)
    zero = GraphAttentionLayer(Fd, D, attention=mode)
    zero.load_state_dict(layer.state_dict(), strict=True)     # no weights of its own: the keys agree
    sd = {"gat." + k: v.detach().clone().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    h_host = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32))
    g_host = torch.from_numpy(rs.standard_normal((N, D)).astype(np.float32))
    layer, zero = layer.to(DEV), zero.to(DEV)
    ctx = torch.from_numpy(ctx_np).to(DEV)
    layer.seed_dropout(seed)
    for call in (1, 2):                                       # every forward draws from the next stream
        layer.zero_grad()
        h = h_host.to(DEV).requires_grad_(True)
        svs = GC.recorded_heads(monkeypatch)
        hp, attn = layer(h, ctx, return_attn_wts=True)
        (hp * g_host.to(DEV)).sum().backward()
        monkeypatch.undo()
        stream = engine.attention_dropout_seed(engine.dropout_base(seed, call), 0, 0)
        assert svs[0]["drop"] == (p, stream) == (p, AD.attention_dropout_seed(AD.dropout_base(seed, call), 0, 0))
        for v in sd.values():
            v.grad = None
        h_ref = h_host.double().requires_grad_(True)
        hp_ref, attn_ref = AD.head(mode, h_ref, torch.from_numpy(ctx_np), sd, keep=AD.keep_mask(p, stream, N, K), p=p,
                                   gate=gates_of(svs[0]))
        (hp_ref * g_host.double()).sum().backward()
        assert relerr(hp.detach().cpu(), hp_ref.detach()) < 1e-5 and relerr(attn.cpu(), attn_ref.detach()) < 1e-5
        assert relerr(h.grad.cpu(), h_ref.grad) < 1e-4
        GC.check_param_grads(layer, sd)
        live = torch.from_numpy(((ctx_np >= 0) & (ctx_np < N)).any(1))
        assert torch.allclose(attn.cpu()[live].sum(1), torch.ones(int(live.sum())), atol=1e-5)      # a distribution
    # eval(): the identity -- the bits of a layer built with rate 0 on the same weights, gradients included
    outs = []
    for m in (layer.eval(), zero.train()):
        m.zero_grad()
        h = h_host.to(DEV).requires_grad_(True)
        hp, attn = m(h, ctx, return_attn_wts=True)
        (hp * g_host.to(DEV)).sum().backward()
        outs.append([hp.detach(), attn, h.grad] + [q.grad for q in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    layer.train()
    layer.attn_drop.eval()                                    # the Dropout alone
    assert torch.equal(layer(h_host.to(DEV), ctx), outs[1][0])


def test_two_heads_by_two_layers_draw_from_four_streams_and_match_the_oracle(monkeypatch):
    rs = np.random.RandomState(17)
    N, Fd, D, K, p, seed = 70, 20, 16, 12, 0.6, 9
    ctx_np = GC.make_table(rs, N, K, out_of_range=False)
    torch.manual_seed(5)
    multi = MultiHeadGraphAttention(Fd, D, 2, 2, attention="gatv2", attention_dropout=p)
    zero = MultiHeadGraphAttention(Fd, D, 2, 2, attention="gatv2")
    zero.load_state_dict(multi.state_dict(), strict=True)
    sd = {"gat." + k: v.detach().clone().double().requires_grad_(True) for k, v in multi.state_dict().items()}
    layers = weights.gat_prefixes(2, 2)
    multi, zero = multi.to(DEV), zero.to(DEV)
    multi.seed_dropout(seed)
    h_host = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32))
    g_host = torch.from_numpy(rs.standard_normal((N, D)).astype(np.float32))
    h, ctx = h_host.to(DEV).requires_grad_(True), torch.from_numpy(ctx_np).to(DEV)
    svs = GC.recorded_heads(monkeypatch)
    out, attn = multi(h, ctx, return_attn_wts=True)
    (out * g_host.to(DEV)).sum().backward()
    monkeypatch.undo()
    base = AD.dropout_base(seed, 1)
    streams = [AD.attention_dropout_seed(base, l, i) for l in range(2) for i in range(2)]
    assert [sv["drop"] for sv in svs] == [(p, s) for s in streams] and len(set(streams)) == 4
    assert streams == [engine.attention_dropout_seed(engine.dropout_base(seed, 1), l, i) for l in range(2) for i in range(2)]
    x = h_ref = h_host.double().requires_grad_(True)
    it = iter(zip(svs, streams))
    for heads in layers:
        outs = []
        for prefix in heads:
            sv, stream = next(it)
            outs.append(AD.head("gatv2", x, torch.from_numpy(ctx_np), sd, prefix, AD.keep_mask(p, stream, N, K), p,
                                gate=gates_of(sv)))
        x = torch.cat([o for o, _ in outs], 1)
    (x * g_host.double()).sum().backward()
    assert relerr(out.detach().cpu(), x.detach()) < 1e-5
    assert relerr(attn[:, 1].cpu(), outs[1][1].detach()) < 1e-5 and torch.allclose(attn.sum(2).cpu(), torch.ones(N, 2), atol=1e-5)
    assert relerr(h.grad.cpu(), h_ref.grad) < 1e-4
    GC.check_param_grads(multi, sd)
    with torch.no_grad():
        assert torch.equal(multi.eval()(h, ctx), zero(h, ctx))


# ---------------------------------------------------------------- 3. the model and the trainer (cova_h64_n11 inputs)
def reference_inputs(**extra):
    fx, cfg, _, batch = load_case("cova_h64_n11")
    cfg = dict(cfg, drop_prob=0.2, **extra)
    sd = weights.seeded_state_dict(int(fx["meta/seed"]), logit_gain=float(fx["meta/logit_gain"]),
                                   **{k: v for k, v in cfg.items() if k not in ("drop_prob", "attention_dropout")})
    return cfg, sd, {k: v.to(DEV) for k, v in batch.items() if torch.is_tensor(v)}, int(fx["meta/img_h"])


@pytest.mark.parametrize("extra", [dict(), dict(n_heads=2, n_gat_layers=2, attention="gatv2", edge_geometry=True)],
                         ids=["reference-head", "2x2-gatv2-edge"])
def test_trainer_gradients_agree_with_the_module_under_the_same_seeds(extra):
    """Same weights, same seed: step 1 of the trainer and forward 1 of the module draw the decoder's and every head's masks
    from the same streams.  The trainer projects with one GEMM per head (adjacent W_i / W_j in its flat bucket) where the
    module issues two, so the gradients agree to GRAD_TOL, not bit for bit."""
    cfg, sd, batch, img_h = reference_inputs(**extra)
    cfg = dict(cfg, attention_dropout=0.5)
    tr = HotPathTrainer(cfg, sd, DEV, dropout_seed=5)
    loss, _ = tr.forward_backward(batch)
    kw = {k: v for k, v in extra.items()}
    m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], cfg["use_context"], cfg["hidden_dim"], cfg["bbox_hidden_dim"],
             cfg["n_additional_feat"], cfg["drop_prob"], None, attention_dropout=0.5, **kw)
    assert list(m.state_dict()) == list(sd)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    m.seed_dropout(5)
    logits = m(batch["images"], batch["bboxes"], batch["additional_feats"], batch["context_indices"])
    heads = [head for layer in logits.grad_fn.sv["gat"] for head in layer["heads"]]
    base = engine.dropout_base(5, 1)
    assert [h["drop"] for h in heads] == [(0.5, engine.attention_dropout_seed(base, l, i))
                                          for l, layer in enumerate(weights.gat_prefixes(cfg.get("n_heads", 1),
                                                                                         cfg.get("n_gat_layers", 1)))
                                          for i in range(len(layer))]
    mloss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"])
    mloss.backward()
    assert abs(float(loss) - float(mloss)) <= 2e-5 * abs(float(mloss))
    ref = {k: q.grad.detach().cpu() for k, q in m.named_parameters()}
    assert all(float(ref[k].abs().max()) > 0 for k in ref if k.startswith("gat.") and not k.endswith("attention_layer.bias"))
    worst = compare_grads({k: v.clone() for k, v in tr.grads.items()}, ref, rtol=GRAD_TOL, outlier_frac=0.0)
    print("worst gradient:", worst)
    # another seed: other masks, another gradient
    other = HotPathTrainer(cfg, sd, DEV, dropout_seed=6)
    other.forward_backward(batch)
    assert not torch.equal(other.grads["gat.W_j.weight" if not extra else "gat.layers.0.heads.0.W_j.weight"],
                           tr.grads["gat.W_j.weight" if not extra else "gat.layers.0.heads.0.W_j.weight"])
    # module eval(): the identity, and the GAT alone in eval mode while the rest trains
    zero = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], cfg["use_context"], cfg["hidden_dim"], cfg["bbox_hidden_dim"],
                cfg["n_additional_feat"], cfg["drop_prob"], None, **kw)
    zero.load_state_dict(m.state_dict(), strict=True)         # (the running statistics m's train forward has left)
    zero = zero.to(DEV)
    args = [batch[k] for k in ("images", "bboxes", "additional_feats", "context_indices")]
    with torch.no_grad():
        assert torch.equal(m.eval()(*args), zero.eval()(*args))
        m.train(), zero.train()
        m.gat.eval()
        m.seed_dropout(3), zero.seed_dropout(3)
        assert torch.equal(m(*args), zero(*args))


def test_predict_is_the_plain_models_and_steps_follow_the_dropout_seed():
    cfg, sd, batch, _ = reference_inputs()
    on = dict(cfg, attention_dropout=0.5)
    a, b, c = HotPathTrainer(on, sd, DEV, dropout_seed=5), HotPathTrainer(on, sd, DEV, dropout_seed=5), \
        HotPathTrainer(on, sd, DEV, dropout_seed=6)
    off = HotPathTrainer(dict(cfg, attention_dropout=0), sd, DEV, dropout_seed=5)
    plain = HotPathTrainer(cfg, sd, DEV, dropout_seed=5)
    assert torch.equal(a.predict(batch)[0], off.predict(batch)[0]) and torch.equal(a.predict(batch)[0], plain.predict(batch)[0])
    assert torch.equal(a.loss(batch), plain.loss(batch))
    rows = attention_rows(a, batch)                           # the export reports the distribution (eval mode)
    assert torch.equal(rows, attention_rows(plain, batch))
    for step in range(3):
        la, lb, lc = a.train_step(batch)[0], b.train_step(batch)[0], c.train_step(batch)[0]
        assert float(la) == float(lb) and torch.equal(a.pbucket.flat, b.pbucket.flat)
        assert torch.equal(a.gbucket.flat, b.gbucket.flat)
        assert not torch.equal(a.gbucket.flat, c.gbucket.flat)
    # rate 0 in the cfg is the trainer without the key, bit for bit; the rate on is another step
    first = HotPathTrainer(on, sd, DEV, dropout_seed=5)
    off.train_step(batch), plain.train_step(batch), first.train_step(batch)
    assert torch.equal(off.pbucket.flat, plain.pbucket.flat) and not torch.equal(first.pbucket.flat, plain.pbucket.flat)
    # the state round-trips: parameters, moments and the step count (which the next step's streams derive from)
    d = HotPathTrainer(on, sd, DEV, dropout_seed=5)
    d.load_state_dict(a.state_dict())
    d.load_optimizer_state_dict(a.optimizer_state_dict())
    assert d.step_count == a.step_count == 3
    assert float(a.train_step(batch)[0]) == float(d.train_step(batch)[0]) and torch.equal(a.pbucket.flat, d.pbucket.flat)
    assert torch.equal(a.predict(batch)[0], d.predict(batch)[0])


def test_cached_features_and_averaged_weights_with_the_option_on():
    """The cached-feature path needs a DeviceDataset: small synthetic pages here (96 x 96), not the fixture's batch."""
    u8, rows = page_set(P=9, seed=4)
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    cfg = dict(CFG, attention_dropout=0.5)
    sd = seeded(CFG)
    kw = dict(frozen=("convnet.",), bn_eval=("convnet.",), dropout_seed=8, average="ema", average_decay=0.5)
    a, b = HotPathTrainer(cfg, sd, DEV, **kw), HotPathTrainer(cfg, sd, DEV, **kw)
    cache = FeatureCache.build(a, ds)
    full, cached = list(ds.batches(3, prefetch=False)), list(ds.batches(3, features=cache))
    assert len(full) == len(cached) == 3 and "images" not in cached[0]
    for fb, cb in zip(full, cached):
        _, calls = profiled(lambda: (a.train_step(fb), b.train_step(cb)))
        assert calls["cova_gat_fwd_drop"] == 2 and calls["cova_gat_bwd_drop"] == 2 and "cova_gat_fwd" not in calls
        assert torch.equal(a.gbucket.flat, b.gbucket.flat) and torch.equal(a.pbucket.flat, b.pbucket.flat)
    plain = HotPathTrainer(CFG, a.averaged_state_dict(), DEV)
    with a.averaged_weights():                                # evaluation on the averaged model: the identity again
        _, calls = profiled(lambda: a.predict(full[0]))
        assert "cova_gat_fwd_drop" not in calls and calls["cova_gat_fwd"] == 1
        assert torch.equal(a.predict(full[0])[0], plain.predict(full[0])[0])
