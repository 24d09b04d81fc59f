"""Every launch path of the layer2 NHWC convolutions (csrc/conv_nhwc.hip) against float64, bit for bit, at the cases of
tests/nhwc_cases.py: both block tiles of the gather kernel in the forward and in the data gradient, all eight geometries of
the contract, the tap planner's edge cases, degenerate maps, joined data gradients, every weight-gradient partition shape,
B = 0, the refusals, and an input beyond 2^31 elements.

Per launch: (1) torch.equal against the float64 reference cast to f32 on integer probes (nhwc_cases: any correct f32
evaluation gives those bits; no tolerance, no element left out); (2) outputs are NaN-filled before the call, so every element
must be written; (3) every output and the workspace, which has exactly cova_conv_nhwc_wgrad_workspace_floats floats, lies
inside a canary-filled buffer that is checked afterwards, and every input is surrounded by NaN; (4) two runs give the same
bits."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib  # noqa: E402
import head_cases as HC  # noqa: E402
import nhwc_cases as NC  # noqa: E402
from helpers import DEV, NAN  # noqa: E402

F32 = torch.float32
GUARD = 64                                      # floats in front of and behind every tensor (keeps 16-byte alignment)
call, query = _lib.call, _lib.query


# ------------------------------------------------------------------------------------------------ buffers
def dev_in(t_nchw):
    """NCHW CPU tensor -> NHWC on the device, NaN in front and behind: a read outside the tensor poisons the result"""
    t = t_nchw.permute(0, 2, 3, 1).contiguous()
    C = t.shape[-1]
    return HC.place(t.reshape(-1, C), C, GUARD, NAN, tail=GUARD, device=DEV)[1]


def dev_mat(t):
    """a 2-D operand (prepared weight) on the device inside NaN"""
    return HC.place(t, t.shape[1], GUARD, NAN, tail=GUARD, device=DEV)[1]


def dev_out(rows, C):
    """(flat, view [rows, C]): an output filled with NaN inside a canary-filled buffer"""
    flat, view = HC.place((rows, C, F32), C, GUARD, HC.CANARY, tail=GUARD, device=DEV)
    view.fill_(NAN)
    return flat, view


def written(flat, view, name):
    """nothing outside ``view`` was touched, everything inside was written"""
    assert HC.untouched(flat, view, view.shape[1]), "%s: written outside the output" % name
    assert not bool(torch.isnan(view).any()), "%s: %d elements not written" % (name, int(torch.isnan(view).sum()))


def all_nan(flat, view, name):
    assert HC.untouched(flat, view, view.shape[1]) and bool(torch.isnan(view).all()), "%s: a refused call wrote" % name


def nchw(view, B, H, W):
    return view.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous().cpu()


def prep(w):
    """OIHW CPU weight -> (forward operand, data-gradient operand), each inside NaN; both are exact permutations"""
    co, ci, k, _ = w.shape
    wf, wd = dev_mat(torch.zeros(k * k * ci, co)), dev_mat(torch.zeros(k * k * co, ci))
    call("cova_conv_nhwc_prep", w.to(DEV), wf, wd, co, ci, k)
    assert torch.equal(wd.cpu(), NC.dgrad_operand(w)) and torch.equal(wf.cpu(), w.permute(2, 3, 1, 0).reshape(k * k * ci, co))
    return wf, wd


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two runs differ"
    return a


def sizes(c):
    return NC.out_size(c.H, c.k, c.s, c.p), NC.out_size(c.W, c.k, c.s, c.p)


# ------------------------------------------------------------------------------------------------ launches
def run_fwd(c, x, wf):
    Ho, Wo = sizes(c)

    def run():
        flat, out = dev_out(c.B * Ho * Wo, c.Co)
        call("cova_conv_nhwc_fwd", x, wf, out, c.B, c.H, c.W, c.Ci, c.Co, c.k, c.s, c.p)
        written(flat, out, "forward")
        return (nchw(out, c.B, Ho, Wo),)
    return twice(run)[0]


def run_dgrad(c, dy, wd, dy2=None, wd1=None, add=None):
    def run():
        flat, dx = dev_out(c.B * c.H * c.W, c.Ci)
        call("cova_conv_nhwc_dgrad", dy, wd, dy2, wd1, add, dx, c.B, c.H, c.W, c.Ci, c.Co, c.k, c.s, c.p)
        written(flat, dx, "data gradient")
        return (nchw(dx, c.B, c.H, c.W),)
    return twice(run)[0]


def run_wgrad(c, x, dy):
    Ho, Wo = sizes(c)
    n = query("cova_conv_nhwc_wgrad_workspace_floats", c.B, Ho, Wo, c.Ci, c.Co, c.k)
    assert n == NC.workspace_floats(c)

    def run():
        fw, dw = dev_out(c.Co, c.Ci * c.k * c.k)
        fs, ws = HC.place((1, n, F32), n, GUARD, HC.CANARY, tail=GUARD, device=DEV)
        call("cova_conv_nhwc_wgrad", x, dy, dw, ws, c.B, c.H, c.W, c.Ci, c.Co, c.k, c.s, c.p)
        written(fw, dw, "weight gradient")
        assert HC.untouched(fs, ws, n), "weight gradient: written outside the workspace"
        return (dw.reshape(c.Co, c.Ci, c.k, c.k).cpu(),)
    return twice(run)[0]


def same(got, ref, c, name):
    ref = ref.float()
    assert got.shape == ref.shape, (name, c, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref) | torch.isnan(got)
        raise AssertionError("%s %s: %d of %d elements differ from float64, first at %s (got %r, want %r)" % (
            name, NC.case_id(c), int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()),
            float(got[bad][0]), float(ref[bad][0])))
    return got.numel()


def check_case(c, wgrad=True):
    """every entry point of one case against float64 -> elements compared"""
    d = NC.probe(c)
    x, dy, add = dev_in(d["x"]), dev_in(d["dy"]), dev_in(d["add"])
    wf, wd = prep(d["w"])
    n = same(run_fwd(c, x, wf), NC.ref_fwd(c, d), c, "forward")
    n += same(run_dgrad(c, dy, wd), NC.ref_dgrad(c, d), c, "data gradient")
    n += same(run_dgrad(c, dy, wd, add=add), NC.ref_dgrad(c, d, addend=True), c, "data gradient + addend")
    if NC.has_joined(c):
        dy2, (_, wd1) = dev_in(d["dy2"]), prep(d["w1"])
        n += same(run_dgrad(c, dy, wd, dy2, wd1), NC.ref_dgrad(c, d, joined=True), c, "joined data gradient")
        n += same(run_dgrad(c, dy, wd, dy2, wd1, add), NC.ref_dgrad(c, d, joined=True, addend=True), c,
                  "joined data gradient + addend")
    if wgrad and NC.has_wgrad(c):
        n += same(run_wgrad(c, x, dy), NC.ref_wgrad(c, d), c, "weight gradient")
    return n


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("group", list(NC.GROUPS), ids=lambda g: "k%ds%dp%d-%dto%d" % g)
def test_every_case_equals_float64_bit_for_bit(group):
    total = 0
    for c in NC.GROUPS[group]:
        print("%s variants: %s" % (NC.case_id(c), NC.variants(c)))
        total += check_case(c)
    print("%d elements compared with torch.equal, 0 excluded" % total)


@pytest.mark.parametrize("c", list(NC.WGRAD_CASES), ids=NC.case_id)
def test_weight_gradient_partitions(c):
    print("%s variants: %s" % (NC.case_id(c), NC.variants(c)))
    assert NC.variants(c)["wgrad"] == NC.WGRAD_CASES[c]
    Ho, Wo = sizes(c)
    assert query("cova_conv_nhwc_wgrad_num_partials", c.B, Ho, Wo, c.Ci, c.Co, c.k) == NC.WGRAD_CASES[c][1]
    check_case(c)


def test_one_by_one_only_gradient_writes_zeros_and_the_addend_at_odd_positions():
    """a 1x1 stride-2 data gradient reaches the even positions only; the three other classes have no tap and are written
    by the same launch: zeros, or the addend alone"""
    for ch in ((64, 128), (128, 64)):
        c = NC.Case(1, 2, 0, ch[0], ch[1], 2, 5, 7)
        d = NC.probe(c)
        _, wd = prep(d["w"])
        dy, add = dev_in(d["dy"]), dev_in(d["add"])
        plain, plus = run_dgrad(c, dy, wd), run_dgrad(c, dy, wd, add=add)
        odd = torch.ones(5, 7, dtype=torch.bool)
        odd[::2, ::2] = False
        assert torch.equal(plain[:, :, odd], torch.zeros_like(plain[:, :, odd]))
        assert torch.equal(plus[:, :, odd], d["add"][:, :, odd])
        assert bool((plain[:, :, ::2, ::2] != 0).any())


@pytest.mark.parametrize("c", NC.EMPTY_CASES, ids=NC.case_id)
def test_empty_batch(c):
    """B = 0: every entry point returns OK; the weight gradient zero-fills dw; nothing else is written"""
    Ho, Wo = sizes(c)
    g = NC._gen(9, *c)
    w = NC.ints((c.Co, c.Ci, c.k, c.k), g)
    wf, wd = prep(w)
    one = dev_in(NC.ints((1, max(c.Ci, c.Co), 1, 1), g))              # a valid pointer; no element of it may be used
    # one pixel of canaries where an output would begin (an empty tensor has no pointer to pass)
    fo, out = HC.place((1, c.Co, F32), c.Co, GUARD, HC.CANARY, tail=GUARD, device=DEV)
    call("cova_conv_nhwc_fwd", one, wf, out, 0, c.H, c.W, c.Ci, c.Co, c.k, c.s, c.p)
    fd, dx = HC.place((1, c.Ci, F32), c.Ci, GUARD, HC.CANARY, tail=GUARD, device=DEV)
    call("cova_conv_nhwc_dgrad", one, wd, None, None, None, dx, 0, c.H, c.W, c.Ci, c.Co, c.k, c.s, c.p)
    call("cova_conv_nhwc_dgrad", one, wd, None, None, one, dx, 0, c.H, c.W, c.Ci, c.Co, c.k, c.s, c.p)
    if NC.has_joined(c):
        call("cova_conv_nhwc_dgrad", one, wd, one, wd, one, dx, 0, c.H, c.W, c.Ci, c.Co, c.k, c.s, c.p)
    torch.cuda.synchronize()
    assert bool((fo == HC.CANARY).all()) and bool((fd == HC.CANARY).all()), "written although B = 0"
    if NC.has_wgrad(c):
        n = query("cova_conv_nhwc_wgrad_workspace_floats", 0, Ho, Wo, c.Ci, c.Co, c.k)
        assert n == NC.workspace_floats(c) == c.k * c.k * c.Ci * c.Co
        fw, dw = dev_out(c.Co, c.Ci * c.k * c.k)
        fs, ws = HC.place((1, n, F32), n, GUARD, HC.CANARY, tail=GUARD, device=DEV)
        call("cova_conv_nhwc_wgrad", one, one, dw, ws, 0, c.H, c.W, c.Ci, c.Co, c.k, c.s, c.p)
        torch.cuda.synchronize()
        assert HC.untouched(fw, dw, dw.shape[1]) and torch.equal(dw, torch.zeros_like(dw))
        assert bool((fs == HC.CANARY).all()), "the workspace was written although B = 0"


# ------------------------------------------------------------------------------------------------ batch independence
def _operands(c, kind):
    if kind == "int":
        return NC.probe(c)
    g = NC._gen(11, *c)
    Ho, Wo = sizes(c)
    d = dict(x=torch.randn(c.B, c.Ci, c.H, c.W, generator=g), w=torch.randn(c.Co, c.Ci, c.k, c.k, generator=g) * 0.05,
             dy=torch.randn(c.B, c.Co, Ho, Wo, generator=g), add=torch.randn(c.B, c.Ci, c.H, c.W, generator=g))
    if NC.has_joined(c):
        d["w1"], d["dy2"] = torch.randn(c.Co, c.Ci, 1, 1, generator=g) * 0.1, torch.randn(c.B, c.Co, Ho, Wo, generator=g)
    return d


INDEPENDENCE = [NC.Case(3, 2, 1, 64, 128, 3, 7, 9), NC.Case(3, 1, 1, 128, 128, 3, 5, 6), NC.Case(1, 2, 0, 64, 128, 4, 6, 5),
                NC.Case(3, 2, 0, 128, 64, 3, 8, 7), NC.Case(3, 1, 2, 192, 64, 2, 3, 4), NC.Case(3, 1, 1, 128, 128, 3, 10, 13)]


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("c", INDEPENDENCE, ids=NC.case_id)
def test_pages_do_not_depend_on_the_batch_around_them(c, kind):
    """The forward and the data gradient of pages [1:] launched alone equal the slice of the whole-batch launch bit for bit
    (the order of the products of a pixel does not depend on where the pixel lies in a block), real-valued operands
    included.  The weight gradient over [0:j) and [j:B), added, equals the whole: exactly on integer probes; on real-valued
    ones both are f32 evaluations of the same sum of M products, each within gamma_M of it (Higham 3.1; one more addition
    for the two halves), so they differ by at most 2 (M + 4) 2^-24 sum|x dy| + one ulp."""
    d = _operands(c, kind)
    rest = c._replace(B=c.B - 1)
    wf, wd = prep(d["w"])
    dev = {k: dev_in(v) for k, v in d.items() if k not in ("w", "w1")}
    tail = {k: dev_in(v[1:]) for k, v in d.items() if k not in ("w", "w1")}
    assert torch.equal(run_fwd(c, dev["x"], wf)[1:], run_fwd(rest, tail["x"], wf))
    assert torch.equal(run_dgrad(c, dev["dy"], wd, add=dev["add"])[1:], run_dgrad(rest, tail["dy"], wd, add=tail["add"]))
    if NC.has_joined(c):
        _, wd1 = prep(d["w1"])
        assert torch.equal(run_dgrad(c, dev["dy"], wd, dev["dy2"], wd1)[1:], run_dgrad(rest, tail["dy"], wd, tail["dy2"], wd1))
    if not NC.has_wgrad(c):
        return
    whole = run_wgrad(c, dev["x"], dev["dy"])
    for j in range(1, c.B):
        a = run_wgrad(c._replace(B=j), dev_in(d["x"][:j]), dev_in(d["dy"][:j]))
        b = run_wgrad(c._replace(B=c.B - j), dev_in(d["x"][j:]), dev_in(d["dy"][j:]))
        if kind == "int":
            assert torch.equal(a + b, whole), j
        else:
            Ho, Wo = sizes(c)
            M = c.B * Ho * Wo
            ref = NC.ref_wgrad(c, d)
            mag = NC.ref_wgrad(c, {k: v.abs() for k, v in d.items()})
            tol = 2 * (M + 4) * HC.U24 * mag + HC.f32_ulp(ref)
            assert bool(((a + b).double() - whole.double()).abs().le(tol).all()), j
            assert HC.violations(whole, ref, mag, M)[0] == 0


# ------------------------------------------------------------------------------------------------ refusals
def _refusal_buffers(B, H, W, Ci, Co, k, s, p):
    """operands and NaN-filled outputs large enough for the call if it were served (C integer division, at least one pixel)"""
    Ho, Wo = max(int((H + 2 * p - k) / s) + 1, 1), max(int((W + 2 * p - k) / s) + 1, 1)
    g = NC._gen(13, B, H, W, Ci, Co, k, s, p)
    kk = max(k, 1) ** 2
    t = dict(x=dev_in(NC.ints((B, Ci, H, W), g)), dy=dev_in(NC.ints((B, Co, Ho, Wo), g)),
             wf=dev_mat(NC.ints((kk * Ci, Co), g)), wd=dev_mat(NC.ints((kk * Co, Ci), g)), wd1=dev_mat(NC.ints((Co, Ci), g)))
    t["out"], t["dx"], t["dw"] = dev_out(B * Ho * Wo, Co), dev_out(B * H * W, Ci), dev_out(Co, Ci * kk)
    t["ws"] = HC.place((1, 4 * kk * Ci * Co, F32), 4 * kk * Ci * Co, GUARD, HC.CANARY, tail=GUARD, device=DEV)
    return t


REFUSED = {                     # name -> (entry points, B, H, W, Ci, Co, k, stride, pad, second source)
    "Ci not a multiple of 64": ("fdw", 2, 5, 6, 96, 128, 3, 1, 1, None),
    "Co not a multiple of 64": ("fdw", 2, 5, 6, 64, 96, 3, 1, 1, None),
    "Ci = 32": ("fdw", 2, 5, 6, 32, 128, 1, 2, 0, None),
    "weight gradient at Co = 64": ("w", 2, 5, 6, 64, 64, 3, 1, 1, None),
    "weight gradient at Co = 192": ("w", 2, 5, 6, 64, 192, 3, 2, 1, None),
    "k = 2": ("fdw", 2, 5, 6, 64, 128, 2, 1, 0, None),
    "stride = 3": ("fdw", 2, 7, 7, 64, 128, 3, 3, 1, None),
    "pad = k (1x1)": ("fdw", 2, 5, 6, 64, 128, 1, 1, 1, None),
    "pad = k (3x3)": ("fdw", 2, 5, 6, 64, 128, 3, 1, 3, None),
    "negative pad": ("fdw", 2, 5, 6, 64, 128, 3, 1, -1, None),
    "dy2 without w2": ("d", 2, 5, 6, 64, 128, 3, 2, 1, "dy2"),
    "w2 without dy2": ("d", 2, 5, 6, 64, 128, 3, 2, 1, "w2"),
    "dy2 on another output grid (3x3 s2 p0)": ("d", 2, 5, 7, 64, 128, 3, 2, 0, "both"),
    "dy2 on another output grid (3x3 s1 p0)": ("d", 2, 5, 7, 64, 128, 3, 1, 0, "both"),
    "dy2 on another output grid (3x3 s1 p2)": ("d", 2, 5, 7, 64, 128, 3, 1, 2, "both"),
    # the map is smaller than the kernel: (H + 2 pad - k) / stride truncates -1 / 2 to 0, so Ho = 1 would pass
    "H + 2 pad < k at stride 2": ("fdw", 2, 2, 5, 64, 128, 3, 2, 0, None),
    "W + 2 pad < k at stride 2": ("fdw", 2, 5, 2, 64, 128, 3, 2, 0, None),
    "H + 2 pad < k at stride 2, 128 -> 64": ("fd", 1, 2, 2, 128, 64, 3, 2, 0, None),
    "H + 2 pad < k at stride 1": ("fdw", 2, 2, 5, 64, 128, 3, 1, 0, None),
    "H = 1 at 3x3 pad 0 stride 2": ("fdw", 2, 1, 5, 64, 128, 3, 2, 0, None),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_before_any_launch(name):
    """each of these raises CovaHipError (COVA_ERR_BAD_ARG) from the argument checks and leaves the NaN-filled outputs and
    the canaries around them untouched"""
    entries, B, H, W, Ci, Co, k, s, p, second = REFUSED[name]
    t = _refusal_buffers(B, H, W, Ci, Co, k, s, p)
    dy2 = t["dy"] if second in ("dy2", "both") else None
    w2 = t["wd1"] if second in ("w2", "both") else None
    if "f" in entries:
        with pytest.raises(_lib.CovaHipError, match="10001"):
            call("cova_conv_nhwc_fwd", t["x"], t["wf"], t["out"][1], B, H, W, Ci, Co, k, s, p)
    if "d" in entries:
        with pytest.raises(_lib.CovaHipError, match="10001"):
            call("cova_conv_nhwc_dgrad", t["dy"], t["wd"], dy2, w2, None, t["dx"][1], B, H, W, Ci, Co, k, s, p)
    if "w" in entries:
        with pytest.raises(_lib.CovaHipError, match="10001"):
            call("cova_conv_nhwc_wgrad", t["x"], t["dy"], t["dw"][1], t["ws"][1], B, H, W, Ci, Co, k, s, p)
    torch.cuda.synchronize()
    for key in ("out", "dx", "dw"):
        all_nan(t[key][0], t[key][1], name)
    assert bool((t["ws"][0] == HC.CANARY).all()), name


def test_the_smallest_served_maps_next_to_the_refused_ones():
    """H + 2 pad = k is served: one output row"""
    for c in (NC.Case(3, 2, 0, 64, 128, 2, 3, 5), NC.Case(3, 2, 0, 128, 64, 1, 3, 3), NC.Case(3, 1, 0, 64, 128, 2, 5, 3),
              NC.Case(3, 2, 1, 64, 128, 2, 1, 1), NC.Case(3, 2, 2, 64, 128, 1, 1, 2)):
        check_case(c)


# ------------------------------------------------------------------------------------------------ beyond 2^31 elements
def _fill_ints(t, g):
    """integers in [-3, 3] into a [B, H, W, C] device tensor, in slabs of rows"""
    B, H, W, C = t.shape
    rows = max((1 << 27) // (W * C), 1)
    for b in range(B):
        for r in range(0, H, rows):
            v = t[b, r:r + rows]
            v.copy_(torch.randint(-3, 4, v.shape, generator=g, device=DEV, dtype=torch.int8))


def _equal_big(a, b):
    """torch.equal of two [B, H, W, C] device tensors in slabs of rows; NaN anywhere fails"""
    assert a.shape == b.shape
    B, H, W, C = a.shape
    rows = max((1 << 27) // (W * C), 1)
    for i in range(B):
        for r in range(0, H, rows):
            if not torch.equal(a[i, r:r + rows], b[i, r:r + rows]):
                return False
    return True


def test_an_input_beyond_2_to_the_31_elements():
    """[2, 5792, 5795, 64]: each page holds 2^31 + 653 312 elements, so every element of the second page lies beyond the
    2^31st.  1x1 stride 2 and 3x3 stride 2 pad 1, 64 -> 128, on integer probes: the whole-batch forward and data gradient
    equal the launches over the two pages alone, whose offsets are small (and which the case table holds to float64); the
    weight gradient, with dy zero except on 50 000 pixels of the first and of the last page (9 * 100 000 < 2^24), equals
    the sum of the two pages' exactly.  The 1x1 data gradient's odd rows and columns of the last page are zeros."""
    L = NC.LARGE
    B, H, W, Ci, Co = L["B"], L["H"], L["W"], L["Ci"], L["Co"]
    assert H * W * Ci > 2 ** 31 and B == 2
    free = torch.cuda.mem_get_info(0)[0]
    assert free > 40 * 2 ** 30, "this test needs 40 GiB of free device memory, %d GiB are free" % (free >> 30)
    g = torch.Generator(device=DEV).manual_seed(20)
    times = {}
    t0 = time.time()
    x = torch.empty(B, H, W, Ci, device=DEV)
    _fill_ints(x, g)
    torch.cuda.synchronize()
    times["input of %d elements" % x.numel()] = time.time() - t0
    operands = {}
    for (k, s, p) in L["geometries"]:
        t0 = time.time()
        Ho, Wo = NC.out_size(H, k, s, p), NC.out_size(W, k, s, p)
        wf, wd = prep(NC.ints((Co, Ci, k, k), NC._gen(21, k)))
        operands[(k, s, p)] = wd
        out = torch.full((B, Ho, Wo, Co), NAN, device=DEV)
        call("cova_conv_nhwc_fwd", x, wf, out, B, H, W, Ci, Co, k, s, p)
        for b in range(B):
            page = torch.full((1, Ho, Wo, Co), NAN, device=DEV)
            call("cova_conv_nhwc_fwd", x[b:b + 1], wf, page, 1, H, W, Ci, Co, k, s, p)
            assert _equal_big(out[b:b + 1], page), ("forward", k, b)
            del page
        torch.cuda.synchronize()
        times["k%d s%d p%d forward" % (k, s, p)] = time.time() - t0
        t0 = time.time()
        dy = out.zero_()
        idx = torch.randperm(Ho * Wo, generator=g, device=DEV)[:L["wgrad_pixels"]]
        for b in (0, B - 1):
            dy[b].view(Ho * Wo, Co)[idx] = torch.randint(-3, 4, (idx.numel(), Co), generator=g, device=DEV).float()
        dws = []
        for (b0, b1) in ((0, B), (0, 1), (B - 1, B)):
            nf = query("cova_conv_nhwc_wgrad_workspace_floats", b1 - b0, Ho, Wo, Ci, Co, k)
            fw, dw = dev_out(Co, Ci * k * k)
            fs, ws = HC.place((1, nf, F32), nf, GUARD, HC.CANARY, tail=GUARD, device=DEV)
            call("cova_conv_nhwc_wgrad", x[b0:b1], dy[b0:b1], dw, ws, b1 - b0, H, W, Ci, Co, k, s, p)
            written(fw, dw, "weight gradient")
            assert HC.untouched(fs, ws, nf)
            dws.append(dw.clone())
        assert torch.equal(dws[0], dws[1] + dws[2]), ("weight gradient", k)
        assert bool((dws[1] != 0).any()) and bool((dws[2] != 0).any()) and not torch.equal(dws[1], dws[2])
        times["k%d s%d p%d weight gradient" % (k, s, p)] = time.time() - t0
        del out, dy
    del x
    for (k, s, p), wd in operands.items():
        t0 = time.time()
        Ho, Wo = NC.out_size(H, k, s, p), NC.out_size(W, k, s, p)
        dy = torch.empty(B, Ho, Wo, Co, device=DEV)
        _fill_ints(dy, g)
        dx = torch.full((B, H, W, Ci), NAN, device=DEV)
        call("cova_conv_nhwc_dgrad", dy, wd, None, None, None, dx, B, H, W, Ci, Co, k, s, p)
        for b in range(B):
            page = torch.full((1, H, W, Ci), NAN, device=DEV)
            call("cova_conv_nhwc_dgrad", dy[b:b + 1], wd, None, None, None, page, 1, H, W, Ci, Co, k, s, p)
            assert _equal_big(dx[b:b + 1], page), ("data gradient", k, b)
            del page
        if k == 1:
            assert not bool(dx[B - 1, 1::2].any()) and not bool(dx[B - 1, :, 1::2].any())
            assert bool(dx[B - 1, H - 2, W - 1].any())
        torch.cuda.synchronize()
        times["k%d s%d p%d data gradient" % (k, s, p)] = time.time() - t0
        del dx, dy
    for key, v in times.items():
        print("%s: %.2f s" % (key, v))
