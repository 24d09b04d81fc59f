"""GPU tests of the page self-attention (CoVA(page_attention_dim=E, page_attention_heads=Hh)): cova_page_attn_fwd /
cova_page_attn_bwd through the C ABI against the float64 torch oracle (tests/page_attn_oracle.py: autograd, no code shared
with the hand-written backward), refusals and empty work, models.PageAttention and the whole model under autograd, and
HotPathTrainer with the option on.

Bounds: the project's own for this layer (tests/test_page_readout_gpu.py, tests/test_gatv2_gpu.py): max-abs error over
max-abs reference below 1e-5 for O and for A (recomputed on the host from the kernel's lse and the f32 qkv), below 1e-4 for
dqkv.  The kernel tests feed qkv: the float64 oracle sees the same f32 values.  The whole model on the cova_h64_n11 inputs
keeps tests/test_model_gpu.py's LOGIT_TOL / LOSS_TOL / GRAD_TOL."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, weights  # noqa: E402
from cova_web_object_detection_amd.evaluation import evaluate_split, fit, predict_split  # noqa: E402
from cova_web_object_detection_amd.features import FeatureCache  # noqa: E402
from cova_web_object_detection_amd.models import CoVA, PageAttention  # noqa: E402
from cova_web_object_detection_amd.pipeline import DeviceDataset  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from helpers import (bits_equal, compare_grads, DEV, framed, GRAD_TOL, GUARD, load_case, LOGIT_TOL,  # noqa: E402
                     LOSS_TOL, padded, profiled, relerr, routing_from_saved, SGEMM_TOL, starts, survived)
from oracle import cova_oracle as O  # noqa: E402
import page_attn_oracle as PA  # noqa: E402
from config_cases import SPLIT_CFG as CFG  # noqa: E402
from trainer_cases import five_steps, n_params, page_set, seeded  # noqa: E402

FWD, BWD = "cova_page_attn_fwd", "cova_page_attn_bwd"
KEY = "page_attention.qkv.weight"


# ---------------------------------------------------------------- 1. the kernels through the C ABI
#        page sizes                E   Hh  pad   (pad: extra floats per row of out / g / dqkv; odd = unaligned rows = scalar stores)
SHAPES = {"one": ((1,), 4, 1, 0),                          # a single row; dh below a lane count
          "ragged": ((37, 0, 1, 5, 0), 8, 2, 3),           # empty pages in the middle and at the end; unaligned out / g rows
          "tiles": ((16, 17, 15, 64, 65), 32, 2, 4),       # one row either side of a 16-row matrix tile and a 64-key LDS tile
          "heads": ((90, 11), 128, 4, 4),                  # the configs[1] page; head column offsets
          "wide": ((300, 2, 130), 256, 2, 8),              # dh = 128; several key tiles
          "long": ((1100, 3), 64, 1, 4),                   # a page longer than any staging
          "limit": ((70,), 512, 4, 0),                     # the channel limit
          # beyond the issue's table: the two launch paths it does not reach
          "partial": ((37, 70), 40, 2, 4),                 # dh = 20: a block of 16 head dims filled in part
          "ninety-six": ((90, 33), 192, 2, 4)}             # dh = 96: the instantiation between dh <= 64 and dh <= 128


def build_case(name, sizes, E, heads, pad, seed):
    rs = np.random.RandomState(seed)
    N = int(sum(sizes))
    return dict(name=name, sizes=tuple(sizes), N=N, B=len(sizes), E=E, heads=heads, pad=pad, ps=starts(sizes),
                qkv=rs.standard_normal((N, 3 * E)).astype(np.float32), g=rs.standard_normal((N, E)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def pa_case(name):
    sizes, E, heads, pad = SHAPES[name]
    case = build_case(name, sizes, E, heads, pad, sum(map(ord, name)))
    case["ref"] = oracle64(case)
    return case


def oracle64(case):
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    qkv = f64(case["qkv"]).requires_grad_(True)
    out, A, lse = PA.attend(qkv, case["ps"], case["heads"])
    (out * f64(case["g"])).sum().backward()
    return dict(out=out.detach().numpy(), lse=lse.detach().numpy(), dqkv=qkv.grad.numpy(),
                A={k: v.detach().numpy() for k, v in A.items()})


def host_probabilities(case, lse):
    """A recomputed from the kernel's lse and the f32 qkv (float64 scores): exp(s_ij - lse_i) per page and head."""
    E, heads, ps = case["E"], case["heads"], case["ps"]
    dh = E // heads
    qkv = case["qkv"].astype(np.float64)
    A = {}
    for p, n in enumerate(case["sizes"]):
        lo, hi = ps[p], ps[p + 1]
        for a in range(heads if n else 0):
            s = qkv[lo:hi, a * dh:(a + 1) * dh] @ qkv[lo:hi, E + a * dh:E + (a + 1) * dh].T / np.sqrt(dh)
            A[(p, a)] = np.exp(s - lse[lo:hi, a:a + 1].astype(np.float64))
    return A


def launch(case):
    """cova_page_attn_fwd + cova_page_attn_bwd on framed buffers -> dict of host arrays (guards checked)."""
    N, B, E, heads, pad = case["N"], case["B"], case["E"], case["heads"], case["pad"]
    qkv = torch.from_numpy(case["qkv"]).to(DEV)
    g = padded(case["g"], E + pad)
    ps = torch.from_numpy(case["ps"]).to(DEV)
    out_b, out = framed(N, E, E + pad)
    lse_b, lse = framed(N, heads, heads)
    d_b, d = framed(N, 3 * E, 3 * E + pad)
    engine.call(FWD, qkv, 3 * E, ps, B, N, E, heads, out, E + pad, lse)
    engine.call(BWD, g, E + pad, qkv, 3 * E, out, E + pad, lse, ps, B, N, E, heads, d, 3 * E + pad)
    torch.cuda.synchronize()
    assert torch.equal(qkv.cpu(), torch.from_numpy(case["qkv"]))
    return dict(out=survived(out_b, N, E), lse=survived(lse_b, N, heads), dqkv=survived(d_b, N, 3 * E))


def errors(got, ref, case):
    errs = {"out": relerr(got["out"], ref["out"]), "dqkv": relerr(got["dqkv"], ref["dqkv"])}
    A = host_probabilities(case, got["lse"])
    errs["A"] = max(relerr(A[k], ref["A"][k]) for k in A)
    return errs


def check_against(got, ref, case, what):
    errs = errors(got, ref, case)
    print(what, {k: "%.2e" % v for k, v in errs.items()})
    for k, e in errs.items():
        assert e < (1e-4 if k == "dqkv" else 1e-5), (what, k, e)


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_backward_match_the_float64_oracle(name):
    case = pa_case(name)
    got, ref = launch(case), case["ref"]            # survived(): guards intact, every row of a page written (no page's
    check_against(got, ref, case, name)             # rows are left out: an empty page has none)
    assert relerr(got["lse"], ref["lse"]) < 1e-5
    ps, E = case["ps"], case["E"]
    for p, n in enumerate(case["sizes"]):
        if n == 1:                                   # one box: O = V exactly, dV = g, no gradient to Q or K
            i = ps[p]
            assert np.array_equal(got["out"][i], case["qkv"][i, 2 * E:])
            assert not got["dqkv"][i, :2 * E].any()
            assert relerr(got["dqkv"][i, 2 * E:], case["g"][i]) < 1e-6
    assert float(np.abs(ref["dqkv"][:, :E]).max()) > 0 or case["N"] == 1


def test_empty_pages_leave_their_rows_unwritten():
    """Rows that no page owns (in front of page_start[0], behind page_start[B], and between nothing: empty pages own none)
    stay NaN in every output while the pages' rows are written."""
    case = pa_case("ragged")
    N, E, heads = case["N"], case["E"], case["heads"]
    lead, trail = 3, 2
    rs = np.random.RandomState(2)
    qkv = np.concatenate([rs.standard_normal((lead, 3 * E)), case["qkv"], rs.standard_normal((trail, 3 * E))]).astype(np.float32)
    g = np.concatenate([rs.standard_normal((lead, E)), case["g"], rs.standard_normal((trail, E))]).astype(np.float32)
    M = N + lead + trail
    ps = torch.from_numpy(case["ps"] + lead).to(DEV)
    out_b, out = framed(M, E, E)
    lse_b, lse = framed(M, heads, heads)
    d_b, d = framed(M, 3 * E, 3 * E)
    qd, gd = torch.from_numpy(qkv).to(DEV), torch.from_numpy(g).to(DEV)
    engine.call(FWD, qd, 3 * E, ps, case["B"], M, E, heads, out, E, lse)
    engine.call(BWD, gd, E, qd, 3 * E, out, E, lse, ps, case["B"], M, E, heads, d, 3 * E)
    torch.cuda.synchronize()
    outside = list(range(lead)) + list(range(lead + N, M))
    got = dict(out=survived(out_b, M, E, unwritten=outside), lse=survived(lse_b, M, heads, unwritten=outside),
               dqkv=survived(d_b, M, 3 * E, unwritten=outside))
    ref = case["ref"]
    assert relerr(got["out"][lead:lead + N], ref["out"]) < 1e-5 and relerr(got["dqkv"][lead:lead + N], ref["dqkv"]) < 1e-4


def spread_case(name):
    """The first row of every page of two or more boxes has its Q scaled until its scores span 210 in the head where they
    span most: exp() of the shifted scores underflows for most keys of that row.  No more than the 200 asked for: the
    check of A recomputes exp(s - lse) in float64 from the kernel's f32 lse, whose own spacing at |lse| in [64, 128) is
    7.6e-6 (twice that above 128), so a wider spread measures the f32 format and not the kernel."""
    base = pa_case(name)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items() if k != "ref"}
    E, heads, ps = case["E"], case["heads"], case["ps"]
    dh = E // heads
    rows = []
    for p, n in enumerate(case["sizes"]):
        if n < 2:
            continue
        i, lo, hi = int(ps[p]), int(ps[p]), int(ps[p + 1])
        q = case["qkv"][i, :E].astype(np.float64)
        spans = []
        for a in range(heads):
            s = case["qkv"][lo:hi, E + a * dh:E + (a + 1) * dh].astype(np.float64) @ q[a * dh:(a + 1) * dh] / np.sqrt(dh)
            spans.append(s.max() - s.min())
        case["qkv"][i, :E] *= np.float32(210.0 / max(spans))
        rows.append((i, lo, hi))
    return case, rows


@pytest.mark.parametrize("name", ["ragged", "heads", "long"])
def test_scores_spread_by_two_hundred_stay_finite_and_within_the_bounds(name):
    case, rows = spread_case(name)
    E, heads = case["E"], case["heads"]
    dh = E // heads
    assert rows
    for i, lo, hi in rows:
        spans = []
        for a in range(heads):
            s = (case["qkv"][lo:hi, E + a * dh:E + (a + 1) * dh].astype(np.float64)
                 @ case["qkv"][i, a * dh:(a + 1) * dh].astype(np.float64) / np.sqrt(dh))
            spans.append(s.max() - s.min())
        assert max(spans) > 200.0
    got = launch(case)
    for k in ("out", "lse", "dqkv"):
        assert np.isfinite(got[k]).all(), k
    check_against(got, oracle64(case), case, name + " (spread)")


@pytest.mark.parametrize("name", ["ragged", "heads", "wide", "long"])
def test_reruns_are_bit_identical(name):
    case = pa_case(name)
    a, b = launch(case), launch(case)
    for k in a:
        assert bits_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["ragged", "tiles", "heads"])
def test_a_page_keeps_its_bits_inside_a_larger_batch(name):
    """The first page alone, and again with three pages in front of it and three behind: O, lse and dqkv of its rows have
    the same bits."""
    full = pa_case(name)
    n, E, heads = full["sizes"][0], full["E"], full["heads"]
    small = build_case(name + "[0]", (n,), E, heads, full["pad"], 1)
    small["qkv"], small["g"] = full["qkv"][:n].copy(), full["g"][:n].copy()
    before, after = (4, 0, 70), (2, 13, 1)
    nb = sum(before)
    big = build_case(name + "+6", before + (n,) + after, E, heads, full["pad"], 5)
    big["qkv"][nb:nb + n], big["g"][nb:nb + n] = small["qkv"], small["g"]
    a, b = launch(small), launch(big)
    for k in ("out", "lse", "dqkv"):
        assert bits_equal(a[k], b[k][nb:nb + n]), k
    check_against(b, oracle64(big), big, name + " inside a larger batch")


def test_entry_points_refuse_bad_arguments_and_skip_empty_work():
    N, B, E, Hh = 8, 2, 16, 2
    full = lambda *shape: torch.full(shape, GUARD, device=DEV)
    ps = torch.tensor([0, 5, 8], dtype=torch.int64, device=DEV)
    qkv, g = torch.randn(N + 1, 3 * E, device=DEV), torch.randn(N, E, device=DEV)
    out, lse, d = full(N, E), full(N, Hh), full(N, 3 * E)
    good_f = [qkv, 3 * E, ps, B, N, E, Hh, out, E, lse]
    good_b = [g, E, qkv, 3 * E, out, E, lse, ps, B, N, E, Hh, d, 3 * E]
    off = qkv.view(-1)[1:]                                    # 4 bytes past a 16-byte boundary; N rows still fit
    assert qkv.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4

    def bad(args, **changes):
        a = list(args)
        for i, v in changes.items():
            a[int(i[1:])] = v
        return a
    for ch in (dict(_6=3), dict(_6=0), dict(_6=-2),                       # Hh does not divide E; no heads
               dict(_5=24, _6=4), dict(_5=8, _6=4),                       # dh = 6, dh = 2: not a multiple of 4 in [4, 128]
               dict(_5=516, _6=6), dict(_5=0), dict(_5=-16),              # E above 512; no channels
               dict(_5=512, _6=2),                                        # dh = 256
               dict(_0=off), dict(_1=3 * E + 2), dict(_1=3 * E - 4),      # a misaligned qkv; ldq % 4; ldq < 3E
               dict(_8=E - 1), dict(_4=-1), dict(_3=-1),                  # ldo below E
               dict(_0=None), dict(_2=None), dict(_7=None), dict(_9=None)):
        with pytest.raises(_lib.CovaHipError, match="10001"):
            engine.call(FWD, *bad(good_f, **ch))
    for ch in (dict(_11=3), dict(_11=0), dict(_10=24, _11=4), dict(_10=516, _11=6), dict(_10=512, _11=2), dict(_10=0),
               dict(_2=off), dict(_3=3 * E + 2), dict(_3=3 * E - 4), dict(_1=E - 1), dict(_5=E - 1), dict(_13=3 * E - 1),
               dict(_9=-1), dict(_8=-1),
               dict(_0=None), dict(_2=None), dict(_4=None), dict(_6=None), dict(_7=None), dict(_12=None)):
        with pytest.raises(_lib.CovaHipError, match="10001"):
            engine.call(BWD, *bad(good_b, **ch))
    # N == 0 or B == 0: nothing is launched, no pointer is needed
    for n, b in ((0, B), (N, 0), (0, 0)):
        engine.call(FWD, None, 3 * E, None, b, n, E, Hh, None, E, None)
        engine.call(BWD, None, E, None, 3 * E, None, E, None, None, b, n, E, Hh, None, 3 * E)
        engine.call(FWD, *bad(good_f, _3=b, _4=n))
        engine.call(BWD, *bad(good_b, _8=b, _9=n))
    torch.cuda.synchronize()
    for t in (out, lse, d):
        assert (t == GUARD).all()
    engine.call(FWD, *good_f)                                   # and the good calls are good
    engine.call(BWD, *good_b)
    torch.cuda.synchronize()
    for t in (out, lse, d):
        assert bool(torch.isfinite(t).all()) and (t != GUARD).all()


# ---------------------------------------------------------------- 2. the module
def test_page_attention_under_autograd_matches_the_oracle():
    rs = np.random.RandomState(13)
    sizes, Fd, E, Hh = (40, 0, 61, 30), 24, 8, 2
    N, ps = sum(sizes), starts(sizes)
    torch.manual_seed(11)
    layer = PageAttention(Fd, E, Hh)
    sd = {"page_attention." + k: v.detach().clone().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    assert list(sd) == [KEY] and sd[KEY].shape == (3 * E, Fd)
    h_host = torch.from_numpy(rs.standard_normal((N, Fd)).astype(np.float32))
    g_host = torch.from_numpy(rs.standard_normal((N, E)).astype(np.float32))
    layer = layer.to(DEV)
    h = h_host.to(DEV).requires_grad_(True)
    out, lse = layer(h, torch.from_numpy(ps).to(DEV), return_lse=True)
    assert out.shape == (N, E) and lse.shape == (N, Hh) and not lse.requires_grad
    sv = out.grad_fn.sv
    (out * g_host.to(DEV)).sum().backward()
    h_ref = h_host.double().requires_grad_(True)
    out_ref, _, lse_ref, qkv_ref = PA.page_attention(h_ref, sd, ps, Hh, return_all=True)
    assert relerr(sv["qkv"].cpu(), qkv_ref.detach()) < SGEMM_TOL
    (out_ref * g_host.double()).sum().backward()
    assert relerr(out.detach().cpu(), out_ref.detach()) < 1e-5
    assert relerr(lse.cpu(), lse_ref.detach()) < 1e-5
    assert relerr(h.grad.cpu(), h_ref.grad) < 1e-4
    assert float(sd[KEY].grad.abs().max()) > 0
    assert relerr(layer.qkv.weight.grad.cpu(), sd[KEY].grad) < 1e-4
    assert layer(h.detach(), torch.from_numpy(ps).to(DEV)).shape == (N, E)
    assert layer(h.detach()[:0], torch.zeros(1, dtype=torch.int64, device=DEV)).shape == (0, E)


# ---------------------------------------------------------------- 3. the whole model
@pytest.mark.parametrize("context", [True, False])
def test_model_with_page_attention_matches_the_oracle_on_the_reference_inputs(monkeypatch, context):
    """The cova_h64_n11 inputs hold ONE page; as in the readout's whole-model test the page is given twice and the last
    five boxes are moved to the copy: the same image, boxes, neighbours and labels as two pages (6 + 5 boxes), so that a
    kernel that attends across pages is caught."""
    fx, cfg, _, b = load_case("cova_h64_n11")
    assert b["images"].shape[0] == 1 and b["bboxes"].shape[0] == 11
    b = dict(b, images=b["images"].repeat(2, 1, 1, 1).contiguous(), bboxes=b["bboxes"].clone())
    b["bboxes"][6:, 0] = 1.0
    E, Hh = 8, 2
    cfg = dict(cfg, use_context=context, page_attention_dim=E, page_attention_heads=Hh)
    # the oracle reaches its gat_stack hook under use_context=True only; without heads in the state dict the patched
    # stack states [own | O], which is the use_context=False head
    ocfg = {k: v for k, v in dict(cfg, use_context=True).items() if not k.startswith("page_attention")}
    wcfg = {k: v for k, v in cfg.items() if k != "drop_prob"}
    seed, gain = int(fx["meta/seed"]), float(fx["meta/logit_gain"])
    sd = weights.seeded_state_dict(seed, logit_gain=gain, **wcfg)
    assert KEY in sd and any(k.startswith("gat.") for k in sd) == context
    img_h = int(fx["meta/img_h"])
    ps = torch.searchsorted(b["bboxes"][:, 0].contiguous(), torch.arange(3, dtype=torch.float32))
    assert ps.tolist() == [0, 6, 11]
    inputs = (b["images"], b["bboxes"], b["additional_feats"], b["context_indices"])
    # the same seed's model without the option (its own state dict: the decoder is narrower)
    pcfg = {k: v for k, v in cfg.items() if not k.startswith("page_attention")}
    plain_sd = weights.seeded_state_dict(seed, logit_gain=gain, **{k: v for k, v in pcfg.items() if k != "drop_prob"})
    plain_ref = O.forward(O.clone_state_dict(plain_sd), *inputs, pcfg, False)
    monkeypatch.setattr(O, "gat_stack", PA.patched_gat_stack(ps, Hh))
    args = [t.to(DEV) for t in inputs]

    def build():
        m = CoVA(cfg["roi_output_size"], img_h, cfg["n_classes"], context, cfg["hidden_dim"], cfg["bbox_hidden_dim"],
                 cfg["n_additional_feat"], cfg["drop_prob"], None, page_attention_dim=E, page_attention_heads=Hh)
        assert [k for k in m.state_dict()] == list(sd)
        missing = m.load_state_dict(sd, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        return m.to(DEV)

    m = build().eval()
    with torch.no_grad():
        logits = m(*args)
    ref = O.forward(O.clone_state_dict(sd), *inputs, ocfg, False)
    assert relerr(logits.cpu(), ref) < LOGIT_TOL
    assert relerr(plain_ref, ref) > 1e-3                       # the option is live
    m = build().train()
    logits = m(*args)
    sv = logits.grad_fn.sv
    assert sv["T"] == sv["F"] + sv["D"] + E and sv["D"] == (cfg["hidden_dim"] if context else 0) and sv["G"] == 0
    assert torch.equal(sv["page_start"].cpu(), ps)             # derived on the device from the page column
    routing = routing_from_saved(sv)                           # forced gates: conv, RoI, decoder and the GAT's slopes
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(logits, b["labels"].to(DEV))
    loss.backward()
    loss_ref, logits_ref, grads_ref, _, inter = O.loss_and_grads(sd, *inputs, b["labels"], ocfg, None, routing)
    e = relerr(sv["page_attn"]["qkv"].cpu(), inter["own"].double() @ sd[KEY].double().T)
    print("qkv against the oracle's projection: %.2e" % e)
    assert e < SGEMM_TOL
    assert relerr(logits.detach().cpu(), logits_ref) < LOGIT_TOL
    assert abs(loss.item() - float(loss_ref)) <= LOSS_TOL * abs(float(loss_ref))
    grads = {k: p.grad for k, p in m.named_parameters()}
    compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0)
    assert float(grads_ref[KEY].abs().max()) > 0               # (compare_grads floors the scale at 1 % of the largest gradient)
    assert relerr(grads[KEY].cpu(), grads_ref[KEY]) < 1e-4


# ---------------------------------------------------------------- 4. the trainer
ACFG = dict(CFG, page_attention_dim=16, page_attention_heads=2)


@pytest.mark.parametrize("kw", [dict(), dict(optimizer="adamw", max_grad_norm=1.0)])
def test_five_steps_with_page_attention_move_its_weight_and_are_reproducible(kw):
    u8, rows = page_set()
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    sd = seeded(ACFG)
    assert sd[KEY].shape == (48, 584)
    a, b = HotPathTrainer(ACFG, sd, DEV, **kw), HotPathTrainer(ACFG, sd, DEV, **kw)
    assert a.params[KEY].shape == (48, 584) and a.grads[KEY].shape == (48, 584)
    T = 584 + 32                                            # the layer's 48 * 584 and a decoder 16 columns wider
    assert sum(v.numel() for v in a.params.values()) == n_params(ACFG) == n_params(CFG) + 48 * 584 + 16 * (2 * T + 16) + 7 * 16
    assert a.pbucket.flat.numel() >= n_params(ACFG) and a.gbucket.flat.numel() == a.pbucket.flat.numel()
    la, sa = five_steps(a, ds)
    lb, sb = five_steps(b, ds)
    assert la == lb and list(sa) == list(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    assert bool(torch.isfinite(sa[KEY]).all())
    for third in range(3):                                                      # the Q, the K and the V rows have moved
        rows16 = slice(16 * third, 16 * third + 16)
        assert not torch.equal(sa[KEY][rows16].cpu(), sd[KEY][rows16]), third
    # checkpoint round trip: parameters, moments and step count into a fresh trainer, then one more identical step
    c = HotPathTrainer(ACFG, sd, DEV, **kw)
    c.load_state_dict(a.state_dict())
    c.load_optimizer_state_dict(a.optimizer_state_dict())
    batch = next(iter(ds.batches(3, prefetch=False)))
    assert float(a.train_step(batch)[0]) == float(c.train_step(batch)[0])
    assert torch.equal(a.pbucket.flat, c.pbucket.flat)
    with pytest.raises(ValueError, match="page_attention_dim"):                 # a checkpoint without the layer
        c.load_state_dict(seeded(CFG))
    with pytest.raises(ValueError, match="page_attention_dim"):                 # and the reverse
        HotPathTrainer(CFG, seeded(CFG), DEV).load_state_dict(a.state_dict())


def test_default_step_issues_none_of_the_new_launches_and_the_option_adds_exactly_its_own():
    u8, rows = page_set(P=3)
    batch = next(iter(DeviceDataset(u8, rows, 2, DEV, spatial_k=6).batches(3, prefetch=False)))
    _, plain = profiled(lambda: HotPathTrainer(CFG, seeded(CFG), DEV).train_step(batch))
    assert not any(n in plain for n in (FWD, BWD))
    off = dict(CFG, page_attention_dim=0, page_attention_heads=4)
    _, again = profiled(lambda: HotPathTrainer(off, seeded(CFG), DEV).train_step(batch))
    assert again == plain
    _, pa = profiled(lambda: HotPathTrainer(ACFG, seeded(ACFG), DEV).train_step(batch))
    added = {k: pa.get(k, 0) - plain.get(k, 0) for k in set(pa) | set(plain) if pa.get(k, 0) != plain.get(k, 0)}
    assert added == {FWD: 1, BWD: 1, "cova_sgemm": 3}, added
    ncfg = dict(ACFG, use_context=False)                                          # independent of use_context
    _, npa = profiled(lambda: HotPathTrainer(ncfg, seeded(ncfg), DEV).train_step(batch))
    assert npa[FWD] == 1 and npa[BWD] == 1 and not any(n.startswith("cova_gat") for n in npa)
    both = dict(ACFG, page_context_dim=16)                                        # and of the readout: each adds its own
    _, nb = profiled(lambda: HotPathTrainer(both, seeded(both), DEV).train_step(batch))
    added = {k: nb.get(k, 0) - plain.get(k, 0) for k in set(nb) | set(plain) if nb.get(k, 0) != plain.get(k, 0)}
    assert added == {FWD: 1, BWD: 1, "cova_page_readout_fwd": 1, "cova_page_readout_bwd": 1, "cova_sgemm": 6}, added


def test_evaluate_split_cached_predict_split_and_fit_with_the_option_on():
    u8, rows = page_set(P=9, seed=4)
    v8, vrows = page_set(P=11, seed=9)
    train, val = DeviceDataset(u8, rows, 2, DEV, spatial_k=6), DeviceDataset(v8, vrows, 2, DEV, spatial_k=6)
    tr = HotPathTrainer(ACFG, seeded(ACFG), DEV, track_metrics=True, frozen=("convnet.",), bn_eval=("convnet.",))
    rep = evaluate_split(tr, val, with_loss=True)
    assert rep.evaluated.all() and rep.ranks.shape == (11, 3) and np.isfinite(rep.loss)
    tcache, vcache = FeatureCache.build(tr, train), FeatureCache.build(tr, val)
    cached, full = next(iter(val.batches(11, features=vcache))), next(iter(val.batches(11, prefetch=False)))
    assert cached.get("images") is None and cached.get("page_start") is not None
    assert torch.equal(tr.predict(cached)[0], tr.predict(full)[0])
    # the batch's table and the one derived from the page column are the same pages
    derived = dict(full)
    derived.pop("page_start")
    assert torch.equal(tr.predict(derived)[0], tr.predict(full)[0])
    plain = HotPathTrainer(CFG, seeded(CFG), DEV)
    assert not torch.equal(tr.predict(full)[0], plain.predict(full)[0])
    stripped = {k: v for k, v in cached.items() if k not in ("images", "page_start")}
    with pytest.raises(ValueError, match="page_attention_dim.*page_start"):
        tr.predict(stripped)
    boxes, _ = predict_split(tr, val)
    assert tuple(boxes.shape) == (11, 3) and int(boxes.min()) >= 0
    before = tr.params[KEY].clone()
    loss = float(tr.train_step(next(iter(train.batches(3, features=tcache))))[0])       # a FeatureCache-fed step
    assert np.isfinite(loss) and not torch.equal(tr.params[KEY], before)
    out = fit(tr, train, val, 2, 3, sampling_fraction=0.9, seed=12, eval_interval=1, train_features=tcache,
              val_features=vcache)
    assert len(out.history) == 2 and out.history[-1]["eval_acc"] is not None


@pytest.mark.parametrize("kw", [dict(accumulate_steps=2), dict(average="ema")])
def test_accumulation_and_averaging_complete_two_steps_with_the_option(kw):
    u8, rows = page_set(P=6)
    ds = DeviceDataset(u8, rows, 2, DEV, spatial_k=6)
    tr = HotPathTrainer(ACFG, seeded(ACFG), DEV, **kw)
    n = n_params(ACFG)
    second = tr.accbucket if "accumulate_steps" in kw else tr.abucket
    assert sum(v.numel() for v in tr.params.values()) == n and KEY in second.views
    assert tr.pbucket.flat.numel() >= n and tr.gbucket.flat.numel() == second.flat.numel() == tr.pbucket.flat.numel()
    before = tr.params[KEY].clone()
    losses = [float(tr.train_step(batch)[0]) for batch in ds.batches(3, prefetch=False)]
    assert len(losses) == 2 and all(np.isfinite(x) for x in losses)
    assert bool(torch.isfinite(tr.pbucket.flat).all()) and bool(torch.isfinite(second.flat).all())
    assert not torch.equal(tr.params[KEY], before)
    if "average" in kw:
        assert bool(torch.isfinite(tr.averaged_state_dict()[KEY]).all())
