"""Every launch path of csrc/conv1x1.hip and csrc/conv1x1_lin.hip on the lattice operands of tests/c11_cases.py
(tests/test_c11_cases_cpu.py proves that the cases reach every instantiation of the host dispatch and every path of the
restated walks, and that the checkers flag a subtly wrong kernel).

Per launch: every operand sits in a buffer with NaN rows in front of row 0 and behind row R - 1 (the kernels clamp to
row R - 1, so a read outside the map poisons a result); every output sits NaN-filled (side_bits: a sentinel word) inside
a guard frame of a full tile of rows, and afterwards every entry inside is written and the frame intact; every launch
runs twice on fresh buffers with bit-equal results; the operands are unchanged.  On the lattice every correct f32
evaluation is exact, so out, side, side_bits, every block's statistics row and their float64 fold, dw and lin are compared
element for element with the float64 references -- there is no tolerance in this file.  The grid cap (option 2) is set
inside try / finally, and the grid the restated walk expects is asserted through cova_conv1x1_num_partials and its
siblings: the capped walks run more than one tile per wave, which the assertion ntiles > 8 * grid states."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))

pytestmark = pytest.mark.gpu

from cova_web_object_detection_amd import _lib  # noqa: E402
import c11_cases as CC  # noqa: E402
from helpers import DEV, GUARD, NAN  # noqa: E402

call, query = _lib.call, _lib.query
F32, F64 = np.float32, np.float64
FRAME = CC.TILE                            # guard rows on either side: a kernel that stores a whole ragged tile stays inside
WORD_FILL, WORD_GUARD, WORD_SENTINEL = 0x55555555, 0x0BADF00D, 0x5EED5EED


class In:
    """an operand [rows, C] (a vector: one row) between FRAME rows of NaN (words: of WORD_FILL)"""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        words = a.dtype == np.uint32
        t = torch.from_numpy(a.view(np.int32) if words else a.astype(F32))
        self.buf = torch.full((a.shape[0] + 2 * FRAME, a.shape[1]), WORD_FILL if words else NAN, dtype=t.dtype, device=DEV)
        self.view = self.buf[FRAME:FRAME + a.shape[0]]
        self.view.copy_(t)
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32))


class Out:
    """an output [rows, cols]: NaN (words: WORD_SENTINEL) inside a frame of GUARD (WORD_GUARD) rows"""

    def __init__(self, rows, cols, words=False):
        self.rows, self.words = rows, words
        self.buf = torch.full((rows + 2 * FRAME, cols), WORD_GUARD if words else GUARD,
                              dtype=torch.int32 if words else torch.float32, device=DEV)
        self.view = self.buf[FRAME:FRAME + rows]
        self.view.fill_(WORD_SENTINEL if words else NAN)

    def frame_intact(self):
        g = WORD_GUARD if self.words else GUARD
        return bool((self.buf[:FRAME] == g).all()) and bool((self.buf[FRAME + self.rows:] == g).all())

    def get(self, what):
        assert self.frame_intact(), "%s: written outside the output" % what
        a = self.view.cpu().numpy()
        if self.words:
            a = a.view(np.uint32)
            assert not (a == WORD_SENTINEL).any(), "%s: a word was not written" % what
        else:
            assert np.isfinite(a).all(), "%s: %d entries were not written (or are not finite)" % (what, int((~np.isfinite(a)).sum()))
        return a

    def untouched(self):
        inner = self.view.view(torch.int32)
        first = inner.flatten()[0]
        return self.frame_intact() and bool((inner == first).all()) and (
            int(first) == WORD_SENTINEL if self.words else bool(torch.isnan(self.view).all()))


@contextlib.contextmanager
def capped(cap):
    """option 2 (the grid cap of every persistent launch) set, and put back to 0 on the way out"""
    assert query("cova_set_option", 2, cap) == 0
    try:
        yield
    finally:
        assert query("cova_set_option", 2, 0) == 0


def twice(run, what):
    """run() -> {name: Out}; launched twice on fresh buffers, bit-equal -> {name: array}"""
    a, b = run(), run()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k].buf.view(torch.int32), b[k].buf.view(torch.int32)), "%s %s: two launches differ" % (what, k)
    return {k: v.get("%s %s" % (what, k)) for k, v in a.items()}


def v(d, k):
    return d[k].view if k in d else None


# ------------------------------------------------------------------------------------------------ conv1x1_kernel
def c11_launch(case, d, nparts, w_trans=0, mask=None):
    s = CC.SPECS[case.spec]
    f, R = s.form, case.R
    mask = s.mask if mask is None else mask
    outs = dict(out=Out(R, f.cout))
    if f.epi in (1, 2):
        outs["part"] = Out(nparts, 2 * f.cout)
    if f.x2:
        outs["part2"] = Out(nparts, 2 * f.cout)
    part = outs["part"].view if "part" in outs else None
    if s.entry == "conv1x1":
        call("cova_conv1x1", v(d, "inp"), v(d, "in2"), v(d, "abc"), case.relu, v(d, "wt" if w_trans else "w"), w_trans,
             v(d, "addend"), v(d, "act") if mask == "act" else None, v(d, "act_bits") if mask == "bits" else None,
             v(d, "msc"), v(d, "msh"), v(d, "z"), v(d, "mean"), v(d, "invstd"), v(d, "z2"), v(d, "mean2"), v(d, "invstd2"),
             outs["out"].view, part, outs["part2"].view if f.x2 else None, R, f.cin, f.cout)
    elif s.entry == "materialize":
        outs["side"] = Out(R, 256)
        if s.bits:
            outs["side_bits"] = Out(R, 8, words=True)
        call("cova_conv1x1_materialize", v(d, "inp"), v(d, "in2"), v(d, "abc"), v(d, "w"), outs["side"].view,
             outs["side_bits"].view if s.bits else None, outs["out"].view, part, R)
    else:                                                        # w [256][64]: the conv's OIHW weight = the logical one transposed
        call("cova_conv1x1_lin_dgrad", v(d, "inp"), v(d, "abc"), v(d, "wt"), v(d, "in3"), v(d, "abc3"), case.relu, v(d, "m"),
             v(d, "cvec"), v(d, "addend"), v(d, "msc"), v(d, "msh"), v(d, "z"), v(d, "mean"), v(d, "invstd"),
             outs["out"].view, part, R)
    return outs


def shaped(got, f, nparts):
    for k in ("part", "part2"):
        if k in got:
            got[k] = got[k].reshape(nparts, 2, f.cout)
    return got


@pytest.mark.parametrize("name", list(CC.SPECS))
def test_conv1x1_kernel_every_walk_is_exact(name):
    s = CC.SPECS[name]
    f = s.form
    for case in CC.c11_cases(name):
        what = "%s R %d cap %d relu %d" % (name, case.R, case.cap, case.relu)
        o = CC.c11_operands(case)
        ref = CC.c11_ref(case, o)
        walk = CC.C11Walk(case.R, case.cap)
        d = {k: In(a) for k, a in o.items()}
        d["wt"] = In(o["w"].T.copy())
        if s.mask == "bits":
            assert np.array_equal(o["act_bits"], CC.pack_bits(o["act"]))
        with capped(case.cap):
            nparts = query("cova_conv1x1_lin_dgrad_num_partials", case.R) if f.ext else \
                query("cova_conv1x1_num_partials", case.R, f.cin, f.cout)
            assert nparts == walk.grid, (what, nparts, walk.grid)          # the grid this case is about is the grid it gets
            if case.cap:
                assert walk.ntiles > CC.NW * walk.grid                     # more than one tile per wave
            base = twice(lambda: c11_launch(case, d, nparts, 1 if f.ext else 0), what)
            others = {}
            if s.entry == "conv1x1":
                others["w_trans 1"] = c11_launch(case, d, nparts, 1)
            if s.mask == "bits":
                others["mask from the map"] = c11_launch(case, d, nparts, 0, "act")
            torch.cuda.synchronize()
        msgs = CC.check_c11(case, shaped(dict(base), f, nparts), ref)
        assert not msgs, "%s: %s" % (what, " | ".join(msgs))
        for tag, outs in others.items():
            for k, out in outs.items():
                assert np.array_equal(out.get("%s %s %s" % (what, tag, k)).view(np.uint32), base[k].view(np.uint32)), \
                    "%s: %s differs from the base launch in %s" % (what, tag, k)
        for k, t in d.items():
            assert t.unchanged(), "%s: operand %s was written" % (what, k)


# ------------------------------------------------------------------------------------------------ weight gradient
class Workspace:
    """a NaN-filled workspace of exactly the floats the library asks for, between two GUARD runs"""
    PAD = 4096

    def __init__(self, floats):
        self.floats = floats
        self.buf = torch.full((floats + 2 * self.PAD,), GUARD, dtype=torch.float32, device=DEV)
        self.view = self.buf[self.PAD:self.PAD + floats]
        self.view.fill_(NAN)

    def frame_intact(self):
        return bool((self.buf[:self.PAD] == GUARD).all()) and bool((self.buf[self.PAD + self.floats:] == GUARD).all())


@pytest.mark.parametrize("name", list(CC.WGRAD_SPECS))
def test_conv1x1_wgrad_every_walk_is_exact(name):
    s = CC.WGRAD_SPECS[name]
    for R, cap in CC.wgrad_walks(name):
        what = "%s R %d cap %d" % (name, R, cap)
        o = CC.wgrad_operands(name, R, cap)
        ref = CC.wgrad_ref(name, o)
        d = {k: In(a) for k, a in o.items()}
        with capped(cap):
            floats = query("cova_conv1x1_wgrad_workspace_floats", R, s.co, s.ci)
            assert floats == (cap or 2 * CC.CUS) * s.co * s.ci, (what, floats)     # the cap in force, two blocks per CU
            if cap:
                assert CC.WgradWalk(R, 1, cap).grid == cap
            ws = Workspace(floats)

            def run():
                dw = Out(s.co, s.ci)
                call("cova_conv1x1_wgrad", v(d, "dz"), v(d, "dz2"), v(d, "dz_abc"), v(d, "act"), v(d, "act_abc"), s.relu,
                     dw.view, ws.view, R, s.co, s.ci)
                return dict(dw=dw)

            got = twice(run, what)
        msgs = CC.check_matrix(got["dw"], ref, what + " dw", "output-channel")
        assert not msgs, " | ".join(msgs)
        assert ws.frame_intact(), what + ": written outside the workspace"
        for k, t in d.items():
            assert t.unchanged(), "%s: operand %s was written" % (what, k)


# ------------------------------------------------------------------------------------------------ the linear form
@pytest.mark.parametrize("name", list(CC.VPROD_SPECS))
def test_conv1x1_vprod_every_walk_is_exact(name):
    s = CC.VPROD_SPECS[name]
    assert query("cova_conv1x1_lin_floats") == CC.LIN_FLOATS
    for R, cap in CC.VPROD_WALKS:
        what = "%s R %d cap %d" % (name, R, cap)
        o = CC.vprod_operands(name, R, cap)
        ref = CC.vprod_ref(name, o)
        d = {k: In(a) for k, a in o.items()}
        with capped(cap):
            floats = query("cova_conv1x1_vprod_workspace_floats", R)
            assert floats == (cap or 2 * CC.CUS) * (256 * 64 + 4 * 64 * 64 + 4 * 64 + 256), (what, floats)
            if cap:
                assert CC.VprodWalk(R, cap).grid == cap
            ws = Workspace(floats)

            def run():
                lin = Out(1, CC.LIN_FLOATS)
                call("cova_conv1x1_vprod", v(d, "v"), v(d, "act"), v(d, "act_abc"), s.relu, lin.view, ws.view, R)
                return dict(lin=lin)

            got = twice(run, what)
        msgs = CC.check_lin(got["lin"][0], ref, what)
        assert not msgs, " | ".join(msgs)
        assert ws.frame_intact(), what + ": written outside the workspace"
        for k, t in d.items():
            assert t.unchanged(), "%s: operand %s was written" % (what, k)


@pytest.mark.parametrize("name", CC.LIN_CASES)
def test_lin_bnsums_and_finish_round_the_double_value_once(name):
    o = CC.lin_operands(name)
    d = {k: In(a) for k, a in o.items()}

    def bnsums():
        part = Out(2, 256)
        call("cova_conv1x1_lin_bnsums", v(d, "lin"), v(d, "w"), v(d, "mean"), v(d, "invstd"), part.view)
        return dict(part=part)

    def finish():
        outs = dict(dw=Out(256, 64), m=Out(64, 64), cvec=Out(1, 64), avec=Out(3, 256))
        call("cova_conv1x1_lin_finish", v(d, "lin"), v(d, "abc"), v(d, "w"), *(outs[k].view for k in ("dw", "m", "cvec", "avec")))
        return outs

    msgs = CC.check_matrix(twice(bnsums, name)["part"], CC.lin_bnsums_ref(o), name + " part")
    got, ref = twice(finish, name), CC.lin_finish_ref(o)
    for k in ("dw", "m", "cvec", "avec"):
        msgs += CC.check_matrix(got[k].reshape(ref[k].shape if ref[k].ndim > 1 else (1, -1)), ref[k].reshape(got[k].shape),
                                "%s %s" % (name, k))
    assert not msgs, " | ".join(msgs)
    for k, t in d.items():
        assert t.unchanged(), "%s: operand %s was written" % (name, k)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_argument_combinations_write_nothing():
    R = 8
    fn = _lib.lib().fn
    stream = torch.cuda.current_stream().cuda_stream
    x = {k: In(np.zeros((R, 256), F32)) for k in ("in", "in2", "addend", "act", "z", "z2", "dz2")}
    vec = {k: In(np.zeros((3, 256), F32)) for k in ("abc", "msc", "msh", "mean", "invstd", "mean2", "invstd2", "cvec")}
    bits = In(np.zeros((R, 8), np.uint32))
    w = In(np.zeros((256, 256), F32))
    ws = Workspace(query("cova_conv1x1_wgrad_workspace_floats", R, 256, 64))

    def p(t, given=1):
        return t.view.data_ptr() if given else None

    for entry, kw in CC.REFUSALS:
        assert CC.form(entry, **kw) == CC.BAD_ARG
        outs = [Out(256, 256) for _ in range(4)]
        o0, o1, o2, o3 = (t.view.data_ptr() for t in outs)
        g = lambda k: kw.get(k, 0)                               # noqa: E731
        if entry == "conv1x1":
            need = kw.get("need", 1)
            rc = fn["cova_conv1x1"](p(x["in"], need), p(x["in2"], g("in2")), p(vec["abc"], g("abc")), 1, p(w), 0,
                                    p(x["addend"], g("addend")), p(x["act"], g("act")), p(bits, g("act_bits")),
                                    p(vec["msc"], g("msc")), p(vec["msh"], g("msc")), p(x["z"], g("z")),
                                    p(vec["mean"], g("mean")), p(vec["invstd"], g("mean")), p(x["z2"], g("z2")),
                                    p(vec["mean2"], g("mean2")), p(vec["invstd2"], g("mean2")), o0 if need else None,
                                    o1 if g("part") else None, o2 if g("mean2") else None, kw.get("R", R), kw["cin"],
                                    kw["cout"], stream)
        elif entry == "materialize":
            rc = fn["cova_conv1x1_materialize"](p(x["in"]), p(x["in2"], kw.get("given", 1)), p(vec["abc"]), p(w), o0, o3, o1,
                                                o2 if kw["part"] else None, kw.get("R", R), stream)
        elif entry == "lin_dgrad":
            rc = fn["cova_conv1x1_lin_dgrad"](p(x["in"]), p(vec["abc"]), p(w), p(x["act"]), p(vec["mean2"]), 1, p(w),
                                              p(vec["cvec"]), p(x["addend"], kw["addend"]), p(vec["msc"], kw.get("given", 1)),
                                              p(vec["msh"]), p(x["z"]), p(vec["mean"]), p(vec["invstd"]), o0, o1,
                                              kw.get("R", R), stream)
        else:
            rc = fn["cova_conv1x1_wgrad"](p(x["in"], kw.get("need", 1)), p(x["dz2"], g("dz2")), p(vec["abc"], g("dz_abc")),
                                          p(x["act"]), None, 0, o0, p(ws), kw.get("R", R), kw["co"], kw["ci"], stream)
        torch.cuda.synchronize()
        assert rc == CC.BAD_ARG, (entry, kw, rc)
        assert all(t.untouched() for t in outs) and ws.frame_intact() and bool(torch.isnan(ws.view).all()), (entry, kw)
