"""The probes of tests/split_probe.py are sensitive: run on a CPU emulation of the bf16 split (torch bfloat16 round-to-nearest
pieces, f32 accumulation), the checkers the GPU tests use pass for the complete six-product split -- in the kernels' order and
in reverse -- and fail for every single-term deletion and for every mis-staged 8-channel slot of one piece.  This is the
evidence that tests/test_split_products_gpu.py would fail for a subtly wrong kernel; it needs no GPU."""
import itertools

import pytest
import torch

import split_probe as sp

SHAPES = [(64, 64), (64, 256), (256, 64)]
R = 256 + 13


def _gen(*key):
    return torch.Generator().manual_seed(1000 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def _probes(cin, cout):
    """every probe of one shape: name -> its launches [(x pieces, w pieces, exact result, K position behind each entry)];
    probe A takes cin / 64 launches to select every input channel once"""
    out = {}
    for n, name in enumerate("ABC"):
        out[name] = []
        for t in range(cin // 64 if name == "A" else 1):
            x, w, ref, k_of = sp.PROBES[name](R, cin, cout, t, _gen(cin, cout, n, t))
            out[name].append((sp.pieces(x), sp.pieces(w), ref, k_of))
    return out


def _failing(probes, terms=sp.TERMS, fx=None, fw=None):
    bad = set()
    for name, launches in probes.items():
        for xp, wp, ref, k_of in launches:
            got = sp.emulate(fx(xp) if fx else xp, fw(wp) if fw else wp, terms)
            if sp.mismatch(got, ref, k_of=k_of) is not None:
                bad.add(name)
    return bad


def test_lattice_pieces_are_exact_and_individually_visible():
    g = _gen(1)
    x = sp.lattice((200000 // 64, 64), g)
    p = sp.pieces(x)
    assert torch.equal((p[0].double() + p[1].double() + p[2].double()).float(), x)
    for order in itertools.permutations(range(3)):          # f32 accumulation in any order returns x bit for bit
        acc = torch.zeros_like(x)
        for i in order:
            acc = acc + p[i]
        assert torch.equal(acc, x), order
    assert float((p[1] != 0).double().mean()) > 0.999 and float((p[2] != 0).double().mean()) > 0.9
    no2 = ((p[0] + p[1]).double() - x.double()).abs() / x.double().abs()
    no1 = ((p[0] + p[2]).double() - x.double()).abs() / x.double().abs()
    assert 1e-6 < float(no2.max()) < 7.7e-6 and 1e-3 < float(no1.max()) < 4e-3
    # a per-channel scale: the exponents of one row span 2^24
    e = torch.frexp(x[0])[1]
    assert int(e.max() - e.min()) >= 20
    q = sp.quarter((1000, 64), g)
    pq = sp.pieces(q)
    assert torch.equal(pq[0] + pq[1], q) and not pq[2].any() and bool((pq[1] != 0).all())
    assert torch.equal(pq[1].abs(), torch.exp2(torch.frexp(pq[0])[1].float() - 10))    # x1 = 2^(k-9), x0 in [2^k, 2^(k+1))
    prod = q.double() * q.flip(0).double()
    assert torch.equal(prod.float().double(), prod)                                      # 20 bits: exact in f32
    x11 = pq[1].double() * pq[1].flip(0).double()
    assert 2.0 ** -20 < float((x11.abs() / prod.abs()).min()) and float((x11.abs() / prod.abs()).max()) < 2.0 ** -18


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_complete_split_passes_every_probe(cin, cout):
    probes = _probes(cin, cout)
    assert _failing(probes) == set()
    assert _failing(probes, tuple(reversed(sp.TERMS))) == set()
    for name, launches in probes.items():
        for xp, wp, ref, k_of in launches:
            sp.check_exact(sp.emulate(xp, wp), ref, name, k_of=k_of)


@pytest.mark.parametrize("cin,cout", SHAPES)
@pytest.mark.parametrize("term,caught_by", [((2, 0), "A"), ((0, 2), "B"), ((1, 1), "C"), ((1, 0), "A"), ((0, 1), "B"),
                                            ((0, 0), "ABC")])
def test_every_single_term_deletion_fails_a_probe(cin, cout, term, caught_by):
    probes = _probes(cin, cout)
    terms = tuple(t for t in sp.TERMS if t != term)
    assert len(terms) == 5
    bad = _failing(probes, terms)
    assert set(caught_by) <= bad, (term, bad)
    name = caught_by[0]
    xp, wp, ref, k_of = probes[name][0]
    with pytest.raises(AssertionError, match="probed entries differ"):
        sp.check_exact(sp.emulate(xp, wp, terms), ref, name, k_of=k_of)


@pytest.mark.parametrize("cin,cout", SHAPES)
@pytest.mark.parametrize("fault", [sp.zero_slot, sp.swap_slot])
@pytest.mark.parametrize("piece", [0, 1, 2])
def test_a_mis_staged_slot_of_one_piece_fails_a_probe(cin, cout, fault, piece):
    probes = _probes(cin, cout)
    for slot in sorted({0, 3, cin // 8 - 1}):
        bad = _failing(probes, fx=lambda pcs: fault(pcs, piece, slot))
        assert "A" in bad, ("x", piece, slot, bad)           # the x pieces: probe A (lattice activations)
        bad = _failing(probes, fw=lambda pcs: fault(pcs, piece, slot))
        assert "B" in bad, ("w", piece, slot, bad)           # the w pieces: probe B (lattice weights)
        if piece < 2:
            assert "C" in bad, ("w", piece, slot, bad)
    # ... and the message names the slot
    xp, wp, ref, k_of = probes["A"][0]
    m = sp.mismatch(sp.emulate(sp.zero_slot(xp, piece, 3), wp), ref, k_of=k_of)
    assert "8-channel slots [3]" in m, m


def test_failure_report_names_tile_and_piece():
    x, w, ref, k_of = sp.probe_a(96, 64, 64, 0, _gen(7))
    xp, wp = sp.pieces(x), sp.pieces(w)
    xp[2][32:64] = 0.0                                       # the third piece of row tile 1 only
    m = sp.mismatch(sp.emulate(xp, wp), ref, k_of=k_of)
    assert "tiles of 32: [1], 1 of them odd" in m and "third piece" in m, m
    got = sp.emulate(sp.pieces(x), wp)
    got[5, 7] = torch.nextafter(got[5, 7], torch.tensor(float("inf")))      # one ulp is a failure
    m = sp.mismatch(got, ref, k_of=k_of)
    assert m is not None and m.startswith("1 of"), m


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_error_class_gate_separates_a_two_piece_product_on_normal_operands(cin, cout):
    """The statistical gate of the GPU test (err <= 2 err(f32 chain) + 2e-7 against fp64) on the CPU emulation: the complete
    split passes, a two-piece / three-product one does not -- for N(0,1) operands.  For one-sign operands the dropped terms
    average out of the metric and the gate cannot tell them apart with any margin: that case is the exact probes'."""
    x, w = sp.operands(2048 + 13, cin, cout, False, cin + cout)
    ref = x.double() @ w.double().t()
    gate = 2.0 * sp.max_err(sp.f32_chain(x, w), ref) + 2e-7
    xp, wp = sp.pieces(x), sp.pieces(w)
    full = sp.max_err(sp.emulate(xp, wp), ref)
    two = sp.max_err(sp.emulate(xp, wp, ((1, 0), (0, 1), (0, 0))), ref)
    print("K = %d: gate %.2e   six products %.2e   two pieces %.2e" % (cin, gate, full, two))
    assert full <= gate < two
    for term in sp.TERMS[:3]:                                # each second-order product on its own is visible too
        e = sp.max_err(sp.emulate(xp, wp, tuple(t for t in sp.TERMS if t != term)), ref)
        assert e > gate, (term, e, gate)
