"""Case table and float64 references for the decoder-tail kernels (csrc/head.hip) and the BatchNorm row kernels
(csrc/bn.hip) off the n_classes = 4, ld = C path.  No GPU import: tests/test_head_cases_cpu.py checks the table itself,
tests/test_head_paths_gpu.py runs it.

``variant(entry, ...)`` restates the HOST dispatch of the two files: which template instantiation a call takes follows
from the shape, the leading dimensions and the 16-byte alignment of the pointers.  Alignment is described by a base
offset in floats from a 16-byte aligned allocation (``None`` = a NULL pointer): ``place()`` slices a larger flat buffer,
so a view at offset 1 keeps 4-byte and loses 16-byte alignment.

Error bound of the sums (``sum_bound``): a sum of L products evaluated in f32 in any order, with or without FMA,
differs from the exact sum by at most gamma_L * sum|a_i b_i|, gamma_L = L u / (1 - L u), u = 2**-24 (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1); (L + 4) u >= gamma_(L+1) for every L used here (L <= 1030), the + 1
being the bias of the forward.  One f32 ulp of the reference is added for the reference's own conversion.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

MAXNC = 16
U24 = 2.0 ** -24
CANARY = 7.0


# ------------------------------------------------------------------------------------------------ dispatch
def _vec4_ok(off, ld):
    """common.h vec4_ok: a NULL pointer passes; otherwise 16-byte aligned and ld % 4 == 0"""
    return off is None or (off % 4 == 0 and ld % 4 == 0)


def variant(entry, **a):
    """The kernel variant the host code of head.hip / bn.hip selects for one call.

    linear_small_fwd (Cin, ldx, x_off, w_off)                  -> "V4" | "V1"
    linear_small_bwd (Cin, ldx, x_off, NC)                     -> ("V4" | "V1", 4 | 16)
    colsum           (C, ldx, x_off)                           -> "V4" | "V1"
    colstats         (C, ldx, x_off)                           -> "reduce64" | "generic"
    bn_bwd_reduce    (C, ldd, d_off, lda, a_off, ldz, z_off)   -> "reduce64" | "generic"      (a_off None: no act)
    bn_act_fwd       (C, ldz, z_off, ldres, res_off, ldo, o_off, scale_off=0, shift_off=0) -> "V4" | "V1"
    bn_bwd_apply     (C, ldd, d_off, lda, a_off, ldz, z_off, lddz, dz_off, lddres, dres_off) -> "V4" | "V1"
    """
    if entry == "linear_small_fwd":
        v4 = a["Cin"] % 4 == 0 and a["ldx"] % 4 == 0 and a["x_off"] % 4 == 0 and a["w_off"] % 4 == 0
        return "V4" if v4 else "V1"
    if entry == "linear_small_bwd":
        if not 0 < a["NC"] <= MAXNC:
            raise ValueError("NC out of range: the entry point refuses it")
        v4 = a["Cin"] % 4 == 0 and a["ldx"] % 4 == 0 and a["x_off"] % 4 == 0
        return ("V4" if v4 else "V1", 4 if a["NC"] <= 4 else MAXNC)
    if entry == "colsum":
        v4 = a["C"] % 4 == 0 and a["ldx"] % 4 == 0 and a["x_off"] % 4 == 0
        return "V4" if v4 else "V1"
    if entry == "colstats":
        return "reduce64" if a["C"] == 64 and a["ldx"] == 64 and _vec4_ok(a["x_off"], a["ldx"]) else "generic"
    if entry == "bn_bwd_reduce":
        no_act = a["a_off"] is None
        fast = (a["C"] == 64 and a["ldd"] == 64 and a["ldz"] == 64 and (no_act or a["lda"] == 64)
                and _vec4_ok(a["d_off"], a["ldd"]) and _vec4_ok(a["z_off"], a["ldz"]) and _vec4_ok(a["a_off"], a["lda"]))
        return "reduce64" if fast else "generic"
    if entry == "bn_act_fwd":
        v4 = (a["C"] % 4 == 0 and _vec4_ok(a["z_off"], a["ldz"]) and _vec4_ok(a["res_off"], a["ldres"])
              and _vec4_ok(a["o_off"], a["ldo"]) and _vec4_ok(a.get("scale_off", 0), 0)
              and _vec4_ok(a.get("shift_off", 0), 0))
        return "V4" if v4 else "V1"
    if entry == "bn_bwd_apply":
        v4 = (a["C"] % 4 == 0 and _vec4_ok(a["d_off"], a["ldd"]) and _vec4_ok(a["a_off"], a["lda"])
              and _vec4_ok(a["z_off"], a["ldz"]) and _vec4_ok(a["dz_off"], a["lddz"])
              and _vec4_ok(a["dres_off"], a["lddres"]))
        return "V4" if v4 else "V1"
    raise KeyError(entry)


# ------------------------------------------------------------------------------------------------ cases
# linear_small: x [N, Cin] with leading dimension Cin + ldx_pad at x_off floats; W [NC, Cin] at w_off (the backward does
# not look at W's alignment: cases with w_off != 0 are forward only)
Linear = collections.namedtuple("Linear", "N Cin NC ldx_pad x_off w_off")


def _lin(N, Cin, NC, ldx_pad=0, x_off=0, w_off=0):
    return Linear(N, Cin, NC, ldx_pad, x_off, w_off)


LINEAR_CASES = [
    # <V4, KN 4>: row batches of 512
    _lin(1, 4, 1), _lin(3, 60, 3), _lin(63, 64, 1), _lin(513, 68, 4), _lin(1030, 68, 1), _lin(1030, 992, 4),
    _lin(1030, 64, 4), _lin(513, 992, 3),
    # <V4, KN 16>: row batches of 128
    _lin(1, 4, 5), _lin(1, 64, 16), _lin(3, 60, 16), _lin(63, 992, 7), _lin(129, 68, 5), _lin(513, 64, 7),
    _lin(1030, 4, 16), _lin(1030, 992, 16),
    # V4 with ldx = Cin + 8
    _lin(129, 64, 4, ldx_pad=8), _lin(63, 60, 3, ldx_pad=8), _lin(1030, 68, 5, ldx_pad=8), _lin(3, 992, 16, ldx_pad=8),
    # <V1, KN 4> by value: row batches of 128
    _lin(1, 1, 1), _lin(3, 5, 3), _lin(63, 63, 1), _lin(129, 65, 4), _lin(513, 65, 1), _lin(1030, 5, 4),
    _lin(1030, 331, 4),
    # <V1, KN 16> by value: row batches of 32
    _lin(1, 1, 16), _lin(1, 5, 5), _lin(3, 63, 7), _lin(129, 65, 16), _lin(513, 5, 5), _lin(63, 331, 16),
    _lin(1030, 65, 16), _lin(1030, 331, 5),
    # V1 by layout at Cin = 64: odd leading dimension, x off by one float, (forward only) W off by one float
    _lin(129, 64, 4, ldx_pad=2), _lin(129, 64, 7, ldx_pad=2), _lin(63, 64, 4, x_off=1), _lin(513, 64, 16, x_off=1),
    _lin(129, 64, 4, w_off=1), _lin(3, 64, 5, w_off=1),
]

# colsum: x [R, C] with leading dimension C + ldx_pad at x_off (V4: 64 row slices; V1: 16)
Colsum = collections.namedtuple("Colsum", "R C ldx_pad x_off")
COLSUM_CASES = [Colsum(*c) for c in (
    (1, 1, 0, 0), (15, 5, 0, 0), (17, 5, 1, 0), (17, 5, 4, 0), (65, 5, 0, 0), (1030, 1, 1, 0), (1030, 5, 0, 0),
    (1, 64, 0, 0), (15, 64, 4, 0), (17, 68, 0, 0), (65, 68, 4, 0), (65, 992, 4, 0), (1030, 64, 0, 0), (1030, 992, 0, 0),
    (17, 64, 1, 0), (1030, 68, 1, 0), (15, 992, 1, 0), (65, 64, 0, 1),
    # scalar kernel on a 16-byte aligned buffer whose rows are padded to a multiple of 4 columns
    (17, 5, 3, 0), (65, 1, 3, 0), (1030, 5, 3, 0),
)]

# ce_sum: N x NC, each run at gscale 1 and 1 / N, with labels, without labels (pred only) and without dlogits
CE_CASES = [(N, NC) for N in (1, 1023, 1025, 2500) for NC in (1, 2, 5, 16)]

# dropout: ldx = C + 3, ldo = C + 2, ldg = C + 1, lddx = C + 2; given and generated masks
DROPOUT_CASES = [(R, C, p) for (R, C) in ((1, 1), (7, 5), (311, 64)) for p in (0.0, 0.2)]

# BatchNorm row kernels: (R, C, relu, res) x layout
BN_SHAPES = [(300, 64, 1, 1), (77, 32, 1, 0), (129, 992, 1, 0), (50, 6, 0, 0), (130, 64, 1, 1)]
# layout -> (pad of every leading dimension, offset of z, offset of every other tensor)
BN_LAYOUTS = collections.OrderedDict([("ld=C", (0, 0, 0)), ("ld=C+4", (4, 0, 0)), ("ld=C+1", (1, 0, 0)),
                                      ("z+1", (0, 1, 0))])
BN_CASES = [(s, l) for s in BN_SHAPES for l in BN_LAYOUTS]


def linear_variants(c):
    """(forward variant, backward variant or None for a forward-only case)"""
    ldx = c.Cin + c.ldx_pad
    fwd = variant("linear_small_fwd", Cin=c.Cin, ldx=ldx, x_off=c.x_off, w_off=c.w_off)
    bwd = None if c.w_off else variant("linear_small_bwd", Cin=c.Cin, ldx=ldx, x_off=c.x_off, NC=c.NC)
    return fwd, bwd


def colsum_variant(c):
    return variant("colsum", C=c.C, ldx=c.C + c.ldx_pad, x_off=c.x_off)


def bn_variants(shape, layout):
    """{entry: variant} of the four BatchNorm row kernels for one case (the test passes act = out iff relu, always dres)"""
    R, C, relu, res = shape
    pad, zoff, off = BN_LAYOUTS[layout]
    ld = C + pad
    a_off = off if relu else None
    return {
        "colstats": variant("colstats", C=C, ldx=ld, x_off=zoff),
        "bn_act_fwd": variant("bn_act_fwd", C=C, ldz=ld, z_off=zoff, ldres=ld, res_off=off if res else None, ldo=ld,
                              o_off=off),
        "bn_bwd_reduce": variant("bn_bwd_reduce", C=C, ldd=ld, d_off=off, lda=ld, a_off=a_off, ldz=ld, z_off=zoff),
        "bn_bwd_apply": variant("bn_bwd_apply", C=C, ldd=ld, d_off=off, lda=ld, a_off=a_off, ldz=ld, z_off=zoff,
                                lddz=ld, dz_off=off, lddres=ld, dres_off=off),
    }


# ------------------------------------------------------------------------------------------------ data
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 10007 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def linear_data(c):
    g = _gen(1, c.N, c.Cin, c.NC)
    return dict(x=torch.randn(c.N, c.Cin, generator=g), W=torch.randn(c.NC, c.Cin, generator=g) * 0.1,
                b=torch.randn(c.NC, generator=g) * 0.1, dy=torch.randn(c.N, c.NC, generator=g))


def colsum_data(c):
    return torch.randn(c.R, c.C, generator=_gen(2, c.R, c.C))


def ce_data(N, NC):
    g = _gen(3, N, NC)
    return torch.randn(N, NC, generator=g) * 4, torch.randint(0, NC, (N,), generator=g)


def dropout_data(R, C):
    g = _gen(4, R, C)
    return dict(x=torch.randn(R, C, generator=g), g=torch.randn(R, C, generator=g),
                keep=(torch.rand(R, C, generator=g) > 0.5).to(torch.uint8))


def bn_data(shape):
    """the distribution of tests/test_kernels_gpu.py::test_batchnorm_train_fwd_bwd"""
    R, C, relu, res = shape
    g = torch.Generator().manual_seed(R + C)
    return dict(x=torch.randn(R, C, generator=g) * 2 + 0.5, gamma=torch.rand(C, generator=g) + 0.5,
                beta=torch.randn(C, generator=g) * 0.1, rm=torch.randn(C, generator=g) * 0.1,
                rv=torch.rand(C, generator=g) + 0.5, resid=torch.randn(R, C, generator=g) if res else None,
                dout=torch.randn(R, C, generator=g))


def place(data, ld, off, fill, tail=8, device="cpu"):
    """A [R, C] tensor laid out with leading dimension ``ld`` at ``off`` floats into a flat buffer that is ``tail``
    elements longer than needed, every element outside the data set to ``fill`` (NaN for inputs: a kernel that reads a
    pad column poisons its sum; CANARY for outputs).  ``data`` = a tensor to copy, or (R, C, dtype) for an output.
    -> (flat buffer, [R, ld] view whose data_ptr() is the pointer to pass)"""
    if isinstance(data, tuple):
        R, C, dtype = data
        data = None
    else:
        (R, C), dtype = data.shape, data.dtype
    assert ld >= C and off >= 0
    flat = torch.full((off + R * ld + tail,), fill, dtype=dtype, device=device)
    view = flat[off:off + R * ld].view(R, ld)
    if data is not None:
        view[:, :C] = data.to(device)
    return flat, view


def untouched(flat, view, C, fill=CANARY):
    """every element of ``flat`` outside view[:, :C] still holds ``fill``"""
    probe = flat.clone()
    off = view.data_ptr() - flat.data_ptr()
    assert off % flat.element_size() == 0
    off //= flat.element_size()
    R, ld = view.shape
    probe[off:off + R * ld].view(R, ld)[:, :C] = fill
    return bool((probe == fill).all())


# ------------------------------------------------------------------------------------------------ float64 references
def linear_fwd_ref(x, W, b):
    x, W, b = x.double(), W.double(), b.double()
    return x @ W.T + b


def linear_fwd_mag(x, W, b):
    """sum_c |x w| + |b|: what the forward's bound scales with (L = Cin)"""
    return x.double().abs() @ W.double().abs().T + b.double().abs()


def linear_bwd_ref(dy, x, W):
    """-> dict(dx, dW, db) and the matching magnitudes (L = NC, N, N)"""
    dy, x, W = dy.double(), x.double(), W.double()
    ref = dict(dx=dy @ W, dW=dy.T @ x, db=dy.sum(0))
    mag = dict(dx=dy.abs() @ W.abs(), dW=dy.abs().T @ x.abs(), db=dy.abs().sum(0))
    return ref, mag


def colsum_ref(x):
    return x.double().sum(0), x.double().abs().sum(0)


def ce_ref(logits, labels, gscale):
    """-> (loss, dlogits) of CrossEntropyLoss(reduction="sum") with the gradient scaled by gscale"""
    l = logits.double()
    lse = torch.logsumexp(l, dim=1)
    loss = (lse - l.gather(1, labels.view(-1, 1)).view(-1)).sum()
    dl = torch.softmax(l, dim=1)
    dl[torch.arange(l.shape[0]), labels] -= 1.0
    return loss, gscale * dl


def dropout_ref(x, keep, p):
    return x.double() * keep.double() / (1.0 - p)


def bn_ref(d, relu):
    """F.batch_norm in float64 (train mode, momentum 0.1, eps 1e-5) + residual + ReLU and its backward for the output
    gradient d["dout"] -> dict(out, running_mean, running_var, dz, dgamma, dbeta, dres)"""
    x = d["x"].double().requires_grad_(True)
    gamma, beta = d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)
    resid = None
    if d["resid"] is not None:
        resid = d["resid"].double().requires_grad_(True)
        y = y + resid
    if relu:
        y = F.relu(y)
    (y * d["dout"].double()).sum().backward()
    dres = resid.grad if resid is not None else d["dout"].double() * ((y > 0) if relu else 1.0)
    return dict(out=y.detach(), running_mean=rm, running_var=rv, dz=x.grad, dgamma=gamma.grad, dbeta=beta.grad,
                dres=dres.detach())


# ------------------------------------------------------------------------------------------------ the bound
def f32_ulp(ref):
    """one unit in the last place of ``ref`` rounded to f32, as float64"""
    r = np.abs(ref.detach().cpu().numpy().astype(np.float32))
    return torch.from_numpy(np.spacing(r).astype(np.float64))


def sum_bound(ref, mag, L):
    return (L + 4) * U24 * mag + f32_ulp(ref)


def violations(got, ref, mag, L):
    """number of elements of ``got`` outside the f32 sum bound around the float64 reference, and the worst error as a
    fraction of its bound"""
    got = got.detach().cpu().double().reshape(ref.shape)
    err, bound = (got - ref).abs(), sum_bound(ref, mag, L)
    bad = ~(err <= bound)                                   # (a NaN is a violation)
    return int(bad.sum()), float((err / bound).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
