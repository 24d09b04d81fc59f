"""The decoder tail (csrc/head.hip) and the BatchNorm row kernels (csrc/bn.hip) off the n_classes = 4, ld = C path: every
host-dispatched kernel variant against a float64 reference at the shapes of tests/head_cases.py.

Per case: (1) the float64 reference with the worst-case bound of an f32 sum (head_cases.sum_bound; nothing tuned), the
tolerances of tests/test_loss_gpu.py for cova_ce_sum and of test_batchnorm_train_fwd_bwd for the BatchNorm kernels;
(2) identities that follow from the code, bit for bit; (3) canaries: every output lies in a buffer that is wider and
longer than what is written, pre-filled with 7.0, and every input carries NaN wherever a correct kernel does not read;
(4) two runs give the same bits.  Then the whole model at n_classes 2, 7, 16 against the oracle, and the refusal of 17."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib, engine, synthetic, weights  # noqa: E402
from cova_web_object_detection_amd.models import CoVA  # noqa: E402
from cova_web_object_detection_amd.trainer import HotPathTrainer  # noqa: E402
from oracle import cova_oracle as O  # noqa: E402
import head_cases as HC  # noqa: E402
from helpers import close, compare_grads, DEV, NAN, GRAD_TOL, LOGIT_TOL, relerr, routing_from_saved  # noqa: E402

F32 = torch.float32
LOSS_GATE, GRAD_GATE = 1e-5, 1e-5               # tests/test_loss_gpu.py: cova_ce_loss_fwd / _bwd with default options
BN_FWD_TOL, BN_GRAD_TOL = 1e-5, 1e-4            # tests/test_kernels_gpu.py::test_batchnorm_train_fwd_bwd


def call(name, *args):
    return _lib.call(name, *args)


def query(name, *args):
    return _lib.query(name, *args)


def dev_in(t, ld=None, off=0):
    """input on the device: NaN in the pad columns and behind the last row"""
    if t.dim() == 1:
        t = t.view(1, -1)
    return HC.place(t, t.shape[1] if ld is None else ld, off, NAN, device=DEV)[1]


def dev_out(R, C, ld=None, off=0, dtype=F32):
    """(flat, view): output buffer pre-filled with the canary"""
    return HC.place((R, C, dtype), C if ld is None else ld, off, HC.CANARY, device=DEV)


def within_bound(got, ref, mag, L, name):
    bad, worst = HC.violations(got, ref, mag, L)
    print("%s: worst |err| / bound = %.3f over %d elements (L = %d)" % (name, worst, ref.numel(), L))
    assert bad == 0, "%s: %d of %d elements outside the f32 sum bound (worst %.3g x the bound)" % (
        name, bad, ref.numel(), worst)


def twice(fn):
    """two runs, bit-equal outputs -> the outputs"""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two runs differ"
    return a


# ------------------------------------------------------------------------------------------------ linear_small
def run_linear_fwd(d, c, NC=None):
    NC = c.NC if NC is None else NC
    ldx = c.Cin + c.ldx_pad
    x, W, b = dev_in(d["x"], ldx, c.x_off), dev_in(d["W"][:NC], c.Cin, c.w_off), dev_in(d["b"][:NC])

    def run():
        flat, y = dev_out(c.N, NC)
        call("cova_linear_small_fwd", x, ldx, W, b, y, c.N, c.Cin, NC)
        assert HC.untouched(flat, y, NC), "logits: written outside [N, NC]"
        return (y.clone(),)
    return twice(run)[0]


def run_linear_bwd(d, c, NC=None, x_off=None):
    """-> dx [N, Cin], dW [NC, Cin], db [NC]"""
    NC = c.NC if NC is None else NC
    x_off = c.x_off if x_off is None else x_off
    ldx, lddx = c.Cin + c.ldx_pad, c.Cin + 2
    x, W = dev_in(d["x"], ldx, x_off), dev_in(d["W"][:NC], c.Cin)
    dy = dev_in(d["dy"][:, :NC].contiguous())

    def run():
        (fx, dx), (fw, dW), (fb, db) = dev_out(c.N, c.Cin, lddx), dev_out(NC, c.Cin), dev_out(1, NC)
        call("cova_linear_small_bwd", dy, x, ldx, W, dx, lddx, dW, db, c.N, c.Cin, NC)
        assert HC.untouched(fx, dx, c.Cin), "dx: written outside [N, Cin]"
        assert HC.untouched(fw, dW, c.Cin) and HC.untouched(fb, db, NC), "dW / db: written outside"
        return dx[:, :c.Cin].clone(), dW.clone(), db.view(-1).clone()
    return twice(run)


@pytest.mark.parametrize("c", HC.LINEAR_CASES, ids=lambda c: "N%d-Cin%d-NC%d-pad%d-x%d-w%d" % c)
def test_linear_small_paths(c):
    d = HC.linear_data(c)
    fwd_v, bwd_v = HC.linear_variants(c)
    print("variants: forward %s, backward %s" % (fwd_v, bwd_v))
    y = run_linear_fwd(d, c)
    within_bound(y, HC.linear_fwd_ref(d["x"], d["W"], d["b"]), HC.linear_fwd_mag(d["x"], d["W"], d["b"]), c.Cin, "logits")
    if c.NC > 4:        # class accumulators are independent: the first four columns are the NC = 4 run's, bit for bit
        assert torch.equal(y[:, :4], run_linear_fwd(d, c, NC=4)), "logits[:, :4] differ from the NC = 4 run"
    if bwd_v is None:
        return
    dx, dW, db = run_linear_bwd(d, c)
    ref, mag = HC.linear_bwd_ref(d["dy"], d["x"], d["W"])
    within_bound(dx, ref["dx"], mag["dx"], c.NC, "dx")
    within_bound(dW, ref["dW"], mag["dW"], c.N, "dW")
    within_bound(db, ref["db"], mag["db"], c.N, "db")
    if c.NC > 4:        # the KN = 16 kernel walks the same rows in the same order per thread as KN = 4
        _, dW4, db4 = run_linear_bwd(d, c, NC=4)
        assert torch.equal(dW[:4], dW4), "dW[:4] differs from the NC = 4 run"
        assert torch.equal(db[:4], db4), "db[:4] differs from the NC = 4 run"
    ldx = c.Cin + c.ldx_pad
    if c.Cin % 4 == 0 and ldx % 4 == 0:     # the same x one float further on: the other V; dx does not depend on V
        other = HC.variant("linear_small_bwd", Cin=c.Cin, ldx=ldx, x_off=1 - c.x_off, NC=c.NC)
        assert other[0] != bwd_v[0] and other[1] == bwd_v[1]
        dx2, dW2, db2 = run_linear_bwd(d, c, x_off=1 - c.x_off)
        assert torch.equal(dx, dx2), "dx depends on the alignment of x"
        assert torch.equal(db, db2), "db depends on the alignment of x"
        within_bound(dW2, ref["dW"], mag["dW"], c.N, "dW (%s)" % other[0])


def test_seventeen_classes_are_refused_before_any_launch():
    c = HC.Linear(5, 64, 17, 0, 0, 0)
    d = HC.linear_data(c)
    x, W, b, dy = dev_in(d["x"]), dev_in(d["W"]), dev_in(d["b"]), dev_in(d["dy"])
    (fy, y), (fx, dx), (fw, dW), (fb, db) = dev_out(5, 17), dev_out(5, 64), dev_out(17, 64), dev_out(1, 17)
    with pytest.raises(_lib.CovaHipError, match="10001"):
        call("cova_linear_small_fwd", x, 64, W, b, y, 5, 64, 17)
    with pytest.raises(_lib.CovaHipError, match="10001"):
        call("cova_linear_small_bwd", dy, x, 64, W, dx, 64, dW, db, 5, 64, 17)
    torch.cuda.synchronize()
    for flat in (fy, fx, fw, fb):
        assert bool((flat == HC.CANARY).all())
    y16 = run_linear_fwd(d, c, NC=16)               # 16 is the last count that is served
    within_bound(y16, HC.linear_fwd_ref(d["x"], d["W"][:16], d["b"][:16]),
                 HC.linear_fwd_mag(d["x"], d["W"][:16], d["b"][:16]), 64, "logits at NC = 16")


# ------------------------------------------------------------------------------------------------ colsum
def colsum_in_kernel_order(x, slices):
    """f32 column sums in the order colsum_kernel takes them: row r goes to slice r % slices (rows of a slice in
    ascending order), then the slices are added in ascending order"""
    R, C = x.shape
    acc = torch.zeros(slices, C, dtype=F32)
    for r0 in range(0, R, slices):
        blk = x[r0:r0 + slices]
        acc[:blk.shape[0]] += blk
    t = torch.zeros(C, dtype=F32)
    for j in range(slices):
        t = t + acc[j]
    return t


@pytest.mark.parametrize("c", HC.COLSUM_CASES, ids=lambda c: "R%d-C%d-pad%d-x%d" % c)
def test_colsum_paths(c):
    x = HC.colsum_data(c)
    ld, v = c.C + c.ldx_pad, HC.colsum_variant(c)
    xv = dev_in(x, ld, c.x_off)

    def run():
        flat, out = dev_out(1, c.C)
        call("cova_colsum", xv, ld, c.R, c.C, out)
        assert HC.untouched(flat, out, c.C), "colsum: written outside [C]"
        return (out.view(-1).clone(),)
    got = twice(run)[0]
    ref, mag = HC.colsum_ref(x)
    within_bound(got, ref, mag, c.R, "colsum %s" % v)
    # plain f32 additions in a fixed order (64 row slices for V = 4, 16 for V = 1): reproducible on the host bit for bit
    assert torch.equal(got.cpu(), colsum_in_kernel_order(x, 64 if v == "V4" else 16)), \
        "colsum %s: not the sum in the kernel's order" % v


# ------------------------------------------------------------------------------------------------ ce_sum
def first_argmax(logits):
    """index of the first maximum of every row (the kernel's strict > scan)"""
    NC = logits.shape[1]
    idx = torch.arange(NC).expand_as(logits)
    return torch.where(logits == logits.max(1, keepdim=True).values, idx, torch.full_like(idx, NC)).min(1).values


@pytest.mark.parametrize("N,NC", HC.CE_CASES)
def test_ce_sum_paths(N, NC):
    logits, labels = HC.ce_data(N, NC)
    lg, lb = dev_in(logits), labels.to(DEV)
    pred_ref = first_argmax(logits)

    def run(gscale, with_labels=True, with_dl=True):
        floss = torch.full((2,), HC.CANARY, device=DEV)
        fdl, dl = dev_out(N, NC)
        fpred = torch.full((N + 8,), 7, dtype=torch.int64, device=DEV)
        call("cova_ce_sum", lg, lb if with_labels else None, N, NC, float(gscale), floss if with_labels else None,
             dl if with_labels and with_dl else None, fpred)
        assert floss[1].item() == HC.CANARY and bool((fpred[N:] == 7).all())
        if with_labels and with_dl:
            assert HC.untouched(fdl, dl, NC), "dlogits: written outside [N, NC]"
        else:
            assert bool((fdl == HC.CANARY).all()), "dlogits written although none was asked for"
        if not with_labels:
            assert floss[0].item() == HC.CANARY
        return floss[:1].clone(), dl.clone(), fpred[:N].clone()

    for gscale in (1.0, 1.0 / N):
        loss_ref, dl_ref = HC.ce_ref(logits, labels, gscale)
        loss, dl, pred = twice(lambda: run(gscale))
        err = abs(loss.item() - float(loss_ref))
        print("N %d NC %d gscale %.3g: loss %r, float64 %r" % (N, NC, gscale, loss.item(), float(loss_ref)))
        assert err <= LOSS_GATE * abs(float(loss_ref)), (loss.item(), float(loss_ref))
        close(dl, dl_ref, GRAD_GATE, "dlogits")
        assert torch.equal(pred.cpu(), pred_ref)
        loss2, _, pred2 = twice(lambda: run(gscale, with_dl=False))
        assert torch.equal(loss2, loss) and torch.equal(pred2, pred)
    _, _, pred3 = twice(lambda: run(1.0, with_labels=False))
    assert torch.equal(pred3.cpu(), pred_ref)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("R,C,p", HC.DROPOUT_CASES)
def test_dropout_paths(R, C, p):
    d = HC.dropout_data(R, C)
    x, g, keep = d["x"], d["g"], d["keep"]
    ldx, ldo, ldg, lddx = C + 3, C + 2, C + 1, C + 2
    # the kernels' arithmetic in f32: inv = 1 / (1 - p) (correctly rounded), one multiplication per element
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    scaled = lambda t, m: torch.where(m.bool(), t * float(inv), torch.zeros(()))      # noqa: E731  (f32 x f32 product)
    assert (x * float(inv)).dtype == F32
    keep_flat = torch.full((R * C + 8,), 7, dtype=torch.uint8, device=DEV)
    keep_flat[:R * C] = keep.view(-1).to(DEV)

    def fwd(xv, ldx_, ldo_, given, seed=0):
        def run():
            flat, out = dev_out(R, C, ldo_)
            if given:
                mflat = keep_flat.clone()
            else:
                mflat = torch.full((R * C + 8,), 7, dtype=torch.uint8, device=DEV)
            call("cova_dropout_fwd", xv, ldx_, out, ldo_, mflat, R, C, float(p), seed, 1 if given else 0)
            assert HC.untouched(flat, out, C), "dropout: written outside [R, C]"
            assert bool((mflat[R * C:] == 7).all()), "mask: written behind R * C"
            return out[:, :C].clone(), mflat[:R * C].view(R, C).clone()
        return twice(run)

    strided, plain = dev_in(x, ldx), dev_in(x)
    out, m = fwd(strided, ldx, ldo, True)
    assert torch.equal(m.cpu(), keep), "a given mask was modified"
    assert torch.equal(out.cpu(), scaled(x, keep))
    ref = HC.dropout_ref(x, keep, p)
    assert bool(((out.cpu().double() - ref).abs() <= 4 * HC.U24 * ref.abs()).all())       # (1 - p), 1 / ., x * .: 3 roundings
    assert torch.equal(fwd(plain, C, C, True)[0], out), "the layout changes the values"
    out_g, m_g = fwd(strided, ldx, ldo, False, seed=1234)
    assert bool((m_g <= 1).all())
    assert torch.equal(out_g.cpu(), scaled(x, m_g.cpu()))
    out_p, m_p = fwd(plain, C, C, False, seed=1234)
    assert torch.equal(m_p, m_g) and torch.equal(out_p, out_g), "the generated mask depends on the layout"
    if p == 0.0:
        assert bool((m_g == 1).all())
    elif R * C >= 1000:
        frac = m_g.float().mean().item()
        assert abs(frac - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / (R * C)), frac
        assert not torch.equal(fwd(strided, ldx, ldo, False, seed=1235)[1], m_g)

    def bwd(gv, ldg_, lddx_):
        def run():
            flat, dx = dev_out(R, C, lddx_)
            call("cova_dropout_bwd", gv, ldg_, keep_flat, dx, lddx_, R, C, float(p))
            assert HC.untouched(flat, dx, C), "dropout backward: written outside [R, C]"
            return (dx[:, :C].clone(),)
        return twice(run)[0]
    dx = bwd(dev_in(g, ldg), ldg, lddx)
    assert torch.equal(dx.cpu(), scaled(g, keep))
    assert torch.equal(bwd(dev_in(g), C, C), dx), "the layout changes the values"
    assert bool((keep_flat[R * C:] == 7).all()) and torch.equal(keep_flat[:R * C].cpu(), keep.view(-1))


# ------------------------------------------------------------------------------------------------ BatchNorm row kernels
@functools.lru_cache(maxsize=None)
def bn_reference(shape):
    d = HC.bn_data(shape)
    return d, HC.bn_ref(d, shape[2])


def bn_tensors(shape, layout):
    R, C, relu, res = shape
    pad, zoff, off = HC.BN_LAYOUTS[layout]
    d, _ = bn_reference(shape)
    ld = C + pad
    return dict(ld=ld, z=dev_in(d["x"], ld, zoff), res=dev_in(d["resid"], ld, off) if res else None,
                dout=dev_in(d["dout"], ld, off), off=off)


def bn_act_fwd(shape, t, scale, shift):
    R, C, relu, res = shape
    ld = t["ld"]

    def run():
        flat, out = dev_out(R, C, ld, t["off"])
        call("cova_bn_act_fwd", t["z"], ld, scale, shift, t["res"], ld if res else 0, out, ld, R, C, relu)
        assert HC.untouched(flat, out, C), "bn_act_fwd: written outside [R, C]"
        return (out,)
    return twice(run)[0]


def bn_bwd_apply(shape, t, act, st, coef):
    R, C, relu, res = shape
    ld = t["ld"]

    def run():
        (fz, dz), (fr, dres) = dev_out(R, C, ld, t["off"]), dev_out(R, C, ld, t["off"])
        call("cova_bn_bwd_apply", t["dout"], ld, act if relu else None, ld, t["z"], ld, st.mean, st.invstd, st.scale, coef,
             dz, ld, dres, ld, R, C)
        assert HC.untouched(fz, dz, C) and HC.untouched(fr, dres, C), "bn_bwd_apply: written outside [R, C]"
        return dz[:, :C].clone(), dres[:, :C].clone()
    return twice(run)


def bn_full(shape, layout):
    """colstats -> finalize -> bn_act_fwd -> bn_backward (reduce, finalize, apply) in one layout"""
    R, C, relu, res = shape
    d, _ = bn_reference(shape)
    t = bn_tensors(shape, layout)
    ld = t["ld"]
    params = {"bn.weight": d["gamma"].to(DEV), "bn.bias": d["beta"].to(DEV)}

    def run():
        buffers = {"bn.running_mean": d["rm"].clone().to(DEV), "bn.running_var": d["rv"].clone().to(DEV),
                   "bn.num_batches_tracked": torch.zeros((), dtype=torch.long, device=DEV)}
        part, n = engine.colstats(t["z"], ld, R, C)
        st = engine.bn_params("bn.", params, buffers, C, t["z"], True, part, n, R)
        flat, out = dev_out(R, C, ld, t["off"])
        call("cova_bn_act_fwd", t["z"], ld, st.scale, st.shift, t["res"], ld if res else 0, out, ld, R, C, relu)
        assert HC.untouched(flat, out, C), "bn_act_fwd: written outside [R, C]"
        (fz, dz), (fr, dres) = dev_out(R, C, ld, t["off"]), dev_out(R, C, ld, t["off"])
        dg, db = engine.bn_backward(t["dout"], ld, out if relu else None, ld, t["z"], ld, st, R, dz, ld, dres, ld)
        assert HC.untouched(fz, dz, C) and HC.untouched(fr, dres, C), "bn_backward: written outside [R, C]"
        assert int(buffers["bn.num_batches_tracked"]) == 1
        run.st, run.out = st, out
        return (out[:, :C].clone(), buffers["bn.running_mean"], buffers["bn.running_var"], dz[:, :C].clone(),
                dres[:, :C].clone(), dg.clone(), db.clone(), part.clone())
    got = twice(run)
    return dict(zip(("out", "running_mean", "running_var", "dz", "dres", "dgamma", "dbeta", "part"), got)), run.st, run.out, t


@functools.lru_cache(maxsize=None)
def bn_base(shape):
    """the ld = C, aligned run of a shape and the coefficients of its backward: what the other layouts must reproduce"""
    R, C, relu, res = shape
    got, st, out, t = bn_full(shape, "ld=C")
    n = query("cova_colreduce_num_chunks", R, C)
    part = torch.empty(n, 2, C, device=DEV)
    call("cova_bn_bwd_reduce", t["dout"], C, out if relu else None, C, t["z"], C, st.mean, st.invstd, R, C, part)
    coef = engine.bn_finalize_bwd(part, n, C, R, None, None, "boxes")
    dz, dres = bn_bwd_apply(shape, t, out, st, coef)
    assert torch.equal(dz, got["dz"]) and torch.equal(dres, got["dres"])       # engine.bn_backward is these three calls
    return got, st, coef


@pytest.mark.parametrize("shape,layout", HC.BN_CASES, ids=lambda v: v if isinstance(v, str) else "R%d-C%d-relu%d-res%d" % v)
def test_bn_row_kernel_paths(shape, layout):
    R, C, relu, res = shape
    print("variants:", HC.bn_variants(shape, layout))
    _, ref = bn_reference(shape)
    got = bn_full(shape, layout)[0] if layout != "ld=C" else bn_base(shape)[0]
    close(got["out"], ref["out"], BN_FWD_TOL, "bn fwd")
    close(got["running_mean"], ref["running_mean"], BN_FWD_TOL, "running_mean")
    close(got["running_var"], ref["running_var"], BN_FWD_TOL, "running_var")
    close(got["dz"], ref["dz"], BN_GRAD_TOL, "bn dz")
    close(got["dres"], ref["dres"], BN_GRAD_TOL, "bn dres")
    close(got["dgamma"], ref["dgamma"], BN_GRAD_TOL, "bn dgamma")
    close(got["dbeta"], ref["dbeta"], BN_GRAD_TOL, "bn dbeta")
    # column statistics: sums of R terms (squares for the second row) held to the f32 sum bound; the partial rows add up
    d, _ = bn_reference(shape)
    x = d["x"].double()
    sums = got["part"].cpu().double().sum(0)
    rows = got["part"].shape[0]
    for i, (r, m) in enumerate(((x.sum(0), x.abs().sum(0)), ((x * x).sum(0), (x * x).sum(0)))):
        err, bound = (sums[i] - r).abs(), (R + rows + 4) * HC.U24 * m + HC.f32_ulp(r)
        assert bool((err <= bound).all()), ("colstats row %d" % i, float((err / bound).max()))
    if layout == "ld=C":
        return
    # the element-wise kernels with the base layout's coefficients: the <4> and <1> forms give the same bits
    base, st, coef = bn_base(shape)
    t = bn_tensors(shape, layout)
    out = bn_act_fwd(shape, t, st.scale, st.shift)
    assert torch.equal(out[:, :C], base["out"]), "bn_act_fwd: the layout changes the values"
    dz, dres = bn_bwd_apply(shape, t, out, st, coef)
    assert torch.equal(dz, base["dz"]), "bn_bwd_apply: the layout changes dz"
    assert torch.equal(dres, base["dres"]), "bn_bwd_apply: the layout changes dres"


# ------------------------------------------------------------------------------------------------ whole model
def model_case(nc, boxes):
    cfg = dict(roi_output_size=(3, 3), n_classes=nc, use_context=True, hidden_dim=48, bbox_hidden_dim=16,
               n_additional_feat=0, drop_prob=0.0)
    wcfg = {k: v for k, v in cfg.items() if k != "drop_prob"}
    sd = weights.seeded_state_dict(len(boxes) * 13 + boxes[0] + nc, logit_gain=2.0, **wcfg)
    batch = synthetic.make_batch(len(boxes), img_h=64, boxes_per_page=boxes, context_size=12, n_classes=nc, seed=boxes[0])
    return cfg, sd, batch


def build_model(cfg, sd):
    m = CoVA(cfg["roi_output_size"], 64, cfg["n_classes"], cfg["use_context"], cfg["hidden_dim"], cfg["bbox_hidden_dim"],
             cfg["n_additional_feat"], cfg["drop_prob"], None)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.to(DEV)


@pytest.mark.parametrize("boxes", [[3, 4], [230]], ids=str)
@pytest.mark.parametrize("nc", [2, 7, 16])
def test_model_with_other_class_counts_matches_oracle(nc, boxes):
    cfg, sd, batch = model_case(nc, boxes)
    m = build_model(cfg, sd)
    args = [batch[k].to(DEV) for k in ("images", "bboxes", "additional_feats", "context_indices")]
    for training in (False, True):
        m.train(training)
        with torch.no_grad():
            got = m(*args)
        assert got.shape == (sum(boxes), nc)
        ref = O.forward(O.clone_state_dict(sd), batch["images"], batch["bboxes"], batch["additional_feats"],
                        batch["context_indices"], cfg, training, None)
        err = relerr(got.cpu(), ref)
        print("n_classes %d boxes %s training %s: logit err %.2e" % (nc, boxes, training, err))
        assert err < LOGIT_TOL, (training, err)
    if nc == 2:
        return
    m = build_model(cfg, sd)
    m.train()
    logits = m(*args)
    routing = routing_from_saved(logits.grad_fn.sv)
    torch.nn.CrossEntropyLoss(reduction="sum")(logits, batch["labels"].to(DEV)).backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    _, _, grads_ref, _, _ = O.loss_and_grads(sd, batch["images"], batch["bboxes"], batch["additional_feats"],
                                             batch["context_indices"], batch["labels"], cfg, None, routing)
    assert grads["decoder.5.weight"].shape[0] == nc
    worst = compare_grads(grads, grads_ref, rtol=GRAD_TOL, outlier_frac=0.0)
    print("n_classes %d boxes %s: worst gradient %s %.2e" % (nc, boxes, worst[0], worst[1]))


def test_trainer_step_with_seven_classes():
    cfg, sd, batch = model_case(7, [20, 11])
    tr = HotPathTrainer(cfg, sd, DEV, track_metrics=True)
    loss, pred = tr.train_step({k: v.to(DEV) for k, v in batch.items() if torch.is_tensor(v)})
    assert math.isfinite(float(loss))
    assert pred.shape == (31,) and int(pred.min()) >= 0 and int(pred.max()) < 7
    buf = tr.metrics.buf
    assert buf.numel() == 7 * 7 + 4
    assert int(buf[:49].sum()) == 31 and int(buf[49]) == 31 and int(buf[50]) == 0
