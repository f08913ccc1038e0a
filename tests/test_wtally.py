"""CPU: the weighted tally circuit (kind 4 / "wtally") -- cell totals against the reference stream and the
closed form, the statement's order, and the Python structure generator held against the independent restatement of
tests/wtally_ref.py by a column-form satisfiability check.  No device."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import wtally_ref as WR

S1W = dict(bits=128, W=64, lb=10, k=11, B=3, wb=3)


def _inputs(bits, B, wb, seed):
    rng = random.Random(seed)
    n = P.synth_paillier_inputs(bits, seed)[0]
    cts = [rng.randrange(1, n * n - 1) for _ in range(B)]
    special = [0, (1 << wb) - 1, 1 << (wb - 1)]          # zero, all ones, a lone top bit
    weights = [special[i] if i < 3 else rng.randrange(1 << wb) for i in range(B)]
    return n, cts, weights


def _closed_form(Ln, W, lb, B, wb):
    from paillier_halo2_amd import layout

    L = 2 * Ln
    mm = layout.mul_mod_cells(L, W, lb)
    asg = lambda nl: layout.assign_cells(nl, W, lb)
    ref = layout.refresh_cells(layout.refresh_aux(W, Ln, Ln), W, lb)
    adv = asg(Ln)[0] + B * asg(L)[0] + B + layout.square_cells(Ln) + ref[0] + B * (2 + 7 * wb - 2 + wb * (2 * mm.advice + 8 * L)) + \
        (B - 1) * mm.advice + asg(L)[0] + layout.assert_equal_cells(L)
    lk = asg(Ln)[1] + B * asg(L)[1] + ref[1] + B * wb * 2 * mm.lookup + (B - 1) * mm.lookup + asg(L)[1]
    return adv, lk


@pytest.mark.parametrize("bits,W,lb,B,wb", [(128, 64, 10, 1, 1), (128, 64, 10, 1, 5), (128, 64, 10, 3, 3), (128, 64, 10, 4, 2), (264, 88, 11, 2, 2)])
def test_layout_totals_equal_the_reference_stream_and_the_closed_form(bits, W, lb, B, wb):
    from paillier_halo2_amd import layout

    n, cts, weights = _inputs(bits, B, wb, 0x3a11 + 16 * B + wb)
    trace = WR.wtally_trace(n, cts, weights, wb)
    root = trace[0]
    want = 1
    for c, w in zip(cts, weights):
        want = want * pow(c, w, n * n) % (n * n)
    assert root == want and len(WR.records(trace[1], trace[2])) == 2 * B * wb + B - 1
    adv, lk, seg = WR.wtally_cells(n, cts, weights, root, wb, bits, W, lb)
    cc = layout.circuit_cells("wtally", bits // W, W, lb, count=B, w_bits=wb)
    assert (cc.advice, cc.lookup) == (len(adv), len(lk)) == _closed_form(bits // W, W, lb, B, wb) and seg["satisfied"]
    for name in ("assign_n", "assign_cts", "weights", "square", "refresh", "chains", "tree", "assign_res", "assert_equal", "end"):
        assert cc.seg[name] == seg[name], name
    assert "load_zero" not in cc.seg and "final" not in cc.seg
    assert cc.seg["square"][0] - cc.seg["weights"][0] == B                 # B consecutive weight cells
    assert WR.wtally_gate_mask(B, wb, bits, W, lb).shape[0] == len(adv)
    assert layout.wtally_tree(B) == WR.wtally_tree(B)


def test_native_cell_counts_and_public_cells_equal_layout():
    """pz_circuit_cells / pz_circuit_public_cells are host logic inside the library: kind 4 carries its shape as n_steps_g = 2 B W,
    n_steps_r = B - 1"""
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    L = pz._lib.lib()
    for bits, W, lb, B, wb in ((128, 64, 10, 3, 3), (128, 64, 10, 1, 1), (128, 64, 10, 1, 64), (264, 88, 11, 2, 2)):
        Ln = bits // W
        a, l = C.c_size_t(), C.c_size_t()
        assert L.pz_circuit_cells(4, Ln, W, lb, 2 * B * wb, B - 1, C.byref(a), C.byref(l)) == 0
        cc = layout.circuit_cells("wtally", Ln, W, lb, count=B, w_bits=wb)
        assert (a.value, l.value) == (cc.advice, cc.lookup)
        npub = C.c_size_t()
        want = Ln + (B + 1) * 2 * Ln + B
        out = np.zeros(want, dtype=np.uint64)
        assert L.pz_circuit_public_cells(4, Ln, W, lb, 2 * B * wb, B - 1, out.ctypes.data, want, C.byref(npub)) == 0 and npub.value == want
        sa = CS.stream_structure("wtally", bits, W, lb, count=B, w_bits=wb)
        assert out.tolist() == sa.public_cells.tolist()
        assert (sa.n_cells, sa.n_steps_g, sa.n_steps_r) == (cc.advice, 2 * B * wb, B - 1)
    INV = pz._lib.PZ_ERR_INVALID
    a = C.c_size_t()
    assert L.pz_circuit_cells(4, 2, 64, 10, 0, 0, C.byref(a), None) == INV              # W = 0
    assert L.pz_circuit_cells(4, 2, 64, 10, 7, 2, C.byref(a), None) == INV              # 2 B does not divide the chain records
    assert L.pz_circuit_cells(4, 2, 64, 10, 2 * 65, 0, C.byref(a), None) == INV         # W = 65
    assert L.pz_circuit_cells(4, 2, 64, 10, 2 * 65537, 65536, C.byref(a), None) == INV  # B = 65537
    assert L.pz_circuit_cells(5, 2, 64, 10, 2, 0, C.byref(a), None) == INV


def test_statement_order_and_length():
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout
    from paillier_halo2_amd import verifier as PV

    bits, W, lb, B, wb = (S1W[f] for f in ("bits", "W", "lb", "B", "wb"))
    Ln = bits // W
    n, cts, weights = _inputs(bits, B, wb, 0x3a12)
    root = WR.wtally_trace(n, cts, weights, wb)[0]
    st = PV.public_inputs("wtally", n, None, root, cts=cts, weights=weights, enc_bits=bits, limb_bits=W)
    assert len(st) == Ln + (B + 1) * 2 * Ln + B == 21 and st == WR.statement(n, cts, weights, root, bits, W)
    assert st[Ln + B * 2 * Ln: Ln + B * 2 * Ln + B] == weights
    # ... and the exposed cells hold exactly these values in the reference stream, in this order
    adv, _, seg = WR.wtally_cells(n, cts, weights, root, wb, bits, W, lb)
    sa = CS.stream_structure("wtally", bits, W, lb, count=B, w_bits=wb)
    assert [adv[c] for c in sa.public_cells.tolist()] == st
    ca = layout.assign_cells(2 * Ln, W, lb)[0]
    want = list(range(Ln)) + [seg["assign_cts"][0] + i * ca + j for i in range(B) for j in range(2 * Ln)] + \
        [seg["weights"][0] + i for i in range(B)] + [seg["assign_res"][0] + j for j in range(2 * Ln)]
    assert sa.public_cells.tolist() == want
    bad = dict(enc_bits=bits, limb_bits=W)
    with pytest.raises(ValueError):
        PV.public_inputs("wtally", n, None, root, cts=cts, **bad)                                   # no weights
    with pytest.raises(ValueError):
        PV.public_inputs("wtally", n, None, root, weights=weights, **bad)                           # no ciphertexts
    with pytest.raises(ValueError):
        PV.public_inputs("wtally", n, None, root, cts=cts, weights=weights[:-1], **bad)             # one weight per ciphertext
    with pytest.raises(ValueError):
        PV.public_inputs("wtally", n, None, root, cts=cts, weights=[1 << 64] + weights[1:], **bad)  # a weight is one 64-bit word
    with pytest.raises(ValueError):
        PV.public_inputs("wtally", n, None, root, cts=[n * n << 1] + cts[1:], weights=weights, **bad)
    with pytest.raises(ValueError):
        PV.public_inputs("tally", n, None, root, cts=cts, weights=weights, **bad)
    # one ciphertext is a statement (mul_scalar)
    assert len(PV.public_inputs("wtally", n, None, root, cts=cts[:1], weights=weights[:1], **bad)) == Ln + 4 * Ln + 1


@pytest.fixture(scope="module")
def s1w_columns():
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k, B, wb = (S1W[f] for f in ("bits", "W", "lb", "k", "B", "wb"))
    sa = CS.stream_structure("wtally", bits, W, lb, count=B, w_bits=wb)
    return sa, CS.columns(sa, k, lb, device="cpu", expose=True), CS.columns(sa, k, lb, device="cpu")


def _placed(cs, starts, n, cts, weights, res, trace=None, instances=None, expose=True):
    bits, W, lb, k, wb = (S1W[f] for f in ("bits", "W", "lb", "k", "wb"))
    adv, lk, _ = WR.wtally_cells(n, cts, weights, res, wb, bits, W, lb, trace)
    inst = None
    if expose:
        inst = WR.statement(n, cts, weights, res, bits, W) if instances is None else instances
    return WR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, inst)


def test_reference_stream_satisfies_the_python_structure(s1w_columns):
    from paillier_halo2_amd import layout

    sa, (cs, starts), (cs0, starts0) = s1w_columns
    bits, W, lb, k, B, wb = (S1W[f] for f in ("bits", "W", "lb", "k", "B", "wb"))
    mask = WR.wtally_gate_mask(B, wb, bits, W, lb)
    assert np.array_equal(sa.gate_mask, mask)
    assert layout.break_points(mask, cs.max_rows).tolist() == starts[: cs.n_adv_used + 1].tolist()
    assert cs.n_instance == 1 and cs0.n_instance == 0 and cs.m == cs0.m + 1 and cs.n_adv_used >= 2     # break points are crossed
    n, cts, weights = _inputs(bits, B, wb, 0x3a13)
    assert weights == [0, 7, 4]
    trace = WR.wtally_trace(n, cts, weights, wb)
    root = trace[0]
    table = range(1 << lb)
    check = lambda cols, c=cs: WR.check_columns(c.selectors, c.map_col, c.map_row, table, cols, c.n_lk)
    assert check(_placed(cs, starts, n, cts, weights, root)) == []
    assert check(_placed(cs0, starts0, n, cts, weights, root, expose=False), cs0) == []                # ... and without the instance column
    # a second weight vector and ciphertext set on the SAME structure
    n_b, cts_b, _ = _inputs(bits, B, wb, 0x3a14)
    w_b = [5, 0, 3]
    assert check(_placed(cs, starts, n_b, cts_b, w_b, WR.wtally_trace(n_b, cts_b, w_b, wb)[0])) == []
    only_copy = lambda bad: bool(bad) and {t for t, _, _ in bad} == {"copy"}
    # a wrong claimed result: only the copy of assert_equal_fresh's bit to the constant 1 fails
    assert only_copy(check(_placed(cs, starts, n, cts, weights, root ^ 2)))
    # a statement weight changed by one; a statement ciphertext limb changed
    Ln = bits // W
    inst = WR.statement(n, cts, weights, root, bits, W)
    inst[Ln + B * 2 * Ln + 1] += 1
    assert only_copy(check(_placed(cs, starts, n, cts, weights, root, instances=inst)))
    inst = WR.statement(n, cts, weights, root, bits, W)
    inst[Ln + 2 * 2 * Ln + 1] += 1
    assert only_copy(check(_placed(cs, starts, n, cts, weights, root, instances=inst)))
    # forged edges: every gate, every lookup and the final equality hold -- only copy constraints object
    for forge in (("weight", 1, 6), ("weight", 0, 1), ("tree", 0, "a", 1), ("tree", 1, "b", 1), ("leaf", 2, 1)):
        ftrace = WR.wtally_trace(n, cts, weights, wb, forge=forge)
        assert ftrace[0] != root, forge
        assert only_copy(check(_placed(cs, starts, n, cts, weights, ftrace[0], trace=ftrace))), forge


def test_one_ciphertext_and_one_bit(s1w_columns):
    """B = 1 (mul_scalar: no tree, the root is the power) and W = 1 (num_to_bits is the bit alone, tied to the weight's cell)"""
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k = (S1W[f] for f in ("bits", "W", "lb", "k"))
    table = range(1 << lb)
    for B, wb, weights in ((1, 1, [1]), (1, 1, [0]), (2, 1, [1, 0]), (1, 4, [9])):
        sa = CS.stream_structure("wtally", bits, W, lb, count=B, w_bits=wb)
        assert np.array_equal(sa.gate_mask, WR.wtally_gate_mask(B, wb, bits, W, lb))
        cs, starts = CS.columns(sa, k, lb, device="cpu", expose=True)
        n, cts, _ = _inputs(bits, B, wb, 0x3a15 + B)
        root = WR.wtally_trace(n, cts, weights, wb)[0]
        if B == 1:
            assert root == pow(cts[0], weights[0], n * n)
        adv, lk, _ = WR.wtally_cells(n, cts, weights, root, wb, bits, W, lb)
        cols = WR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, WR.statement(n, cts, weights, root, bits, W))
        assert WR.check_columns(cs.selectors, cs.map_col, cs.map_row, table, cols, cs.n_lk) == []
        # the chain run with the other bit: the weight cell's copy constraint objects
        ftrace = WR.wtally_trace(n, cts, weights, wb, forge=("weight", 0, weights[0] ^ 1))
        adv, lk, _ = WR.wtally_cells(n, cts, weights, ftrace[0], wb, bits, W, lb, ftrace)
        cols = WR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, WR.statement(n, cts, weights, ftrace[0], bits, W))
        bad = WR.check_columns(cs.selectors, cs.map_col, cs.map_row, table, cols, cs.n_lk)
        assert bad and {t for t, _, _ in bad} == {"copy"}


def test_refusals():
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    for B, wb in ((None, 3), (0, 3), (65537, 3), (3, None), (3, 0), (3, 65)):
        with pytest.raises(ValueError):
            layout.circuit_cells("wtally", 2, 64, 10, count=B, w_bits=wb)
        with pytest.raises(ValueError):
            CS.stream_structure("wtally", 128, 64, 10, count=B, w_bits=wb)
    with pytest.raises(ValueError):
        layout.circuit_cells("tally", 2, 64, 10, count=3, w_bits=3)
    with pytest.raises(ValueError):
        layout.circuit_cells("wtally", 2, 64, 10, n_steps_g=5, count=3, w_bits=3)
    with pytest.raises(ValueError):
        CS.stream_structure("tally", 128, 64, 10, count=3, w_bits=3)
    with pytest.raises(ValueError):
        CS.stream_structure("add", 128, 64, 10, w_bits=3)
    # n_public = Ln + (B + 1) 2 Ln + B must fit the instance column's usable rows (as for the tally): B = 500, W = 1 exposes 2506 values
    # and break_rows = 2039 holds fewer (the cut itself is made at k = 15 so that the stream fits a handful of columns)
    sa = CS.stream_structure("wtally", 128, 64, 10, count=500, w_bits=1)
    assert len(sa.public_cells) == 2 + 501 * 4 + 500
    with pytest.raises(ValueError):
        CS.columns(sa, 15, 10, device="cpu", expose=True, break_rows=2039)
