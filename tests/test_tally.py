"""CPU: the tally circuit (kind 3 / "tally") -- cell totals, the statement's order, and the Python structure
generator held against the independent restatement of tests/tally_ref.py by a column-form satisfiability check.  No device."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import tally_ref as TR

S1 = dict(bits=128, W=64, lb=10, k=11, B=5)


def _inputs(bits, B, seed):
    rng = random.Random(seed)
    n = P.synth_paillier_inputs(bits, seed)[0]
    cts = [rng.randrange(1, n * n) for _ in range(B)]
    return n, cts


@pytest.mark.parametrize("bits,W,lb,B", [(128, 64, 10, 2), (128, 64, 10, 5), (128, 64, 10, 6), (128, 64, 10, 7), (264, 88, 11, 3)])
def test_layout_totals_equal_the_reference_stream(bits, W, lb, B):
    from paillier_halo2_amd import layout

    n, cts = _inputs(bits, B, 0x7a11 + B)
    root, steps = TR.tally_trace(n, cts)
    want = 1
    for c in cts:
        want = want * c % (n * n)
    assert root == want and len(steps) == B - 1
    adv, lk, seg = TR.tally_cells(n, cts, root, bits, W, lb)
    cc = layout.circuit_cells("tally", bits // W, W, lb, count=B)
    assert (cc.advice, cc.lookup) == (len(adv), len(lk)) and seg["satisfied"]
    for name in ("assign_n", "assign_cts", "square", "refresh", "tree", "assign_res", "assert_equal", "end"):
        assert cc.seg[name] == seg[name], name
    assert "load_zero" not in cc.seg and "final" not in cc.seg
    assert TR.tally_gate_mask(B, bits, W, lb).shape[0] == len(adv)
    assert layout.tally_tree(B) == TR.tally_tree(B)


def test_issue_table_counts():
    from paillier_halo2_amd import layout

    cc = layout.circuit_cells("tally", 2, 64, 10, count=5)
    rb = layout.row_budget(11)
    assert (cc.advice, cc.lookup, rb.columns_for(cc.advice), rb.columns_for(cc.lookup)) == (6221, 944, 4, 1)
    cc = layout.circuit_cells("tally", 32, 64, 16, count=64)
    rb = layout.row_budget(17)
    assert (rb.columns_for(cc.advice), rb.columns_for(cc.lookup)) == (32, 1)


def test_native_cell_counts_and_public_cells_equal_layout():
    """pz_circuit_cells / pz_circuit_public_cells are host logic inside the library: kind 3 with the count carried as n_steps_g = B - 1"""
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    L = pz._lib.lib()
    for bits, W, lb, B in ((128, 64, 10, 5), (264, 88, 11, 3)):
        Ln = bits // W
        a, l = C.c_size_t(), C.c_size_t()
        assert L.pz_circuit_cells(3, Ln, W, lb, B - 1, 0, C.byref(a), C.byref(l)) == 0
        cc = layout.circuit_cells("tally", Ln, W, lb, count=B)
        assert (a.value, l.value) == (cc.advice, cc.lookup)
        npub = C.c_size_t()
        want = Ln + (B + 1) * 2 * Ln
        out = np.zeros(want, dtype=np.uint64)
        assert L.pz_circuit_public_cells(3, Ln, W, lb, B - 1, 0, out.ctypes.data, want, C.byref(npub)) == 0 and npub.value == want
        sa = CS.stream_structure("tally", bits, W, lb, count=B)
        assert out.tolist() == sa.public_cells.tolist()
    INV = pz._lib.PZ_ERR_INVALID
    a = C.c_size_t()
    assert L.pz_circuit_cells(3, 2, 64, 10, 0, 0, C.byref(a), None) == INV          # fewer than two ciphertexts
    assert L.pz_circuit_cells(3, 2, 64, 10, 4, 1, C.byref(a), None) == INV          # a tally has no second chain
    assert L.pz_circuit_cells(3, 2, 64, 10, 65536, 0, C.byref(a), None) == INV      # more than 65536
    assert L.pz_circuit_cells(4, 2, 64, 10, 0, 0, C.byref(a), None) == INV


def test_statement_order_and_length():
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout
    from paillier_halo2_amd import verifier as PV

    bits, W, lb, B = S1["bits"], S1["W"], S1["lb"], S1["B"]
    Ln = bits // W
    n, cts = _inputs(bits, B, 0x7a12)
    root, _ = TR.tally_trace(n, cts)
    st = PV.public_inputs("tally", n, None, root, cts=cts, enc_bits=bits, limb_bits=W)
    assert len(st) == Ln + (B + 1) * 2 * Ln == 26 and st == TR.statement(n, cts, root, bits, W)
    # ... and the exposed cells hold exactly these values in the reference stream, in this order
    adv, _, seg = TR.tally_cells(n, cts, root, bits, W, lb)
    sa = CS.stream_structure("tally", bits, W, lb, count=B)
    assert [adv[c] for c in sa.public_cells.tolist()] == st
    ca = layout.assign_cells(2 * Ln, W, lb)[0]
    want = list(range(Ln)) + [seg["assign_cts"][0] + i * ca + j for i in range(B) for j in range(2 * Ln)] + \
        [seg["assign_res"][0] + j for j in range(2 * Ln)]
    assert sa.public_cells.tolist() == want
    with pytest.raises(ValueError):
        PV.public_inputs("tally", n, None, root, enc_bits=bits, limb_bits=W)
    with pytest.raises(ValueError):
        PV.public_inputs("tally", n, None, root, cts=cts[:1], enc_bits=bits, limb_bits=W)
    with pytest.raises(ValueError):
        PV.public_inputs("tally", n, None, root, cts=[n * n << 1] + cts[1:], enc_bits=bits, limb_bits=W)
    with pytest.raises(ValueError):
        PV.public_inputs("add", n, 1, root, 1, 2, cts=cts, enc_bits=bits, limb_bits=W)


@pytest.fixture(scope="module")
def s1_columns():
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k, B = (S1[f] for f in ("bits", "W", "lb", "k", "B"))
    sa = CS.stream_structure("tally", bits, W, lb, count=B)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=True)
    return sa, cs, starts


def _placed(cs, starts, n, cts, res, steps=None, instances=None):
    bits, W, lb, k = (S1[f] for f in ("bits", "W", "lb", "k"))
    adv, lk, _ = TR.tally_cells(n, cts, res, bits, W, lb, steps)
    inst = TR.statement(n, cts, res, bits, W) if instances is None else instances
    return TR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, inst)


def test_reference_stream_satisfies_the_python_structure(s1_columns):
    from paillier_halo2_amd import layout

    sa, cs, starts = s1_columns
    bits, W, lb, k, B = (S1[f] for f in ("bits", "W", "lb", "k", "B"))
    mask = TR.tally_gate_mask(B, bits, W, lb)
    assert np.array_equal(sa.gate_mask, mask)
    assert layout.break_points(mask, cs.max_rows).tolist() == starts[: cs.n_adv_used + 1].tolist()
    assert (cs.n_adv, cs.n_lk, cs.m, cs.n_instance) == (4, 1, 7, 1) and cs.n_adv_used >= 2     # break points are crossed
    n, cts = _inputs(bits, B, 0x7a13)
    root, steps = TR.tally_trace(n, cts)
    table = range(1 << lb)
    check = lambda cols: TR.check_columns(cs.selectors, cs.map_col, cs.map_row, table, cols, cs.n_lk)
    assert check(_placed(cs, starts, n, cts, root)) == []
    # a wrong claimed product: only the copy of assert_equal_fresh's bit to the constant 1 (and nothing else) fails
    bad = check(_placed(cs, starts, n, cts, root ^ 2))
    assert bad and {t for t, _, _ in bad} == {"copy"}
    # a statement that differs from the witness in one limb of c_3
    inst = TR.statement(n, cts, root, bits, W)
    inst[2 + 2 * 4 + 1] += 1
    bad = check(_placed(cs, starts, n, cts, root, instances=inst))
    assert bad and {t for t, _, _ in bad} == {"copy"}
    # forged edges: every gate, every lookup and the final equality hold -- only the tree's copy constraints object
    for forge in ((B // 2, "a", 1), (0, "b", 1)):        # the first level-1 block's a = r_0 + 1; level 0's b = c_2 + 1
        froot, fsteps = TR.tally_trace(n, cts, forge=forge)
        assert froot != root
        bad = check(_placed(cs, starts, n, cts, froot, steps=fsteps))
        assert bad and {t for t, _, _ in bad} == {"copy"}, forge


def test_refusals():
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    for B in (None, 0, 1, 65537):
        with pytest.raises(ValueError):
            layout.circuit_cells("tally", 2, 64, 10, count=B)
    with pytest.raises(ValueError):
        layout.circuit_cells("add", 2, 64, 10, count=3)
    with pytest.raises(ValueError):
        CS.stream_structure("tally", 128, 64, 10)
    with pytest.raises(ValueError):
        CS.stream_structure("tally", 128, 64, 10, count=1)
    with pytest.raises(ValueError):
        CS.stream_structure("add", 128, 64, 10, count=2)
    # n_public = Ln + (B + 1) 2 Ln must fit the instance column's usable rows: B = 600 exposes 2406 values, and break_rows = 2039 (k = 11's
    # usable rows, passed explicitly: the cut itself is made at k = 14 so that the 600 ciphertexts fit a handful of columns) holds fewer
    sa = CS.stream_structure("tally", 128, 64, 10, count=600)
    assert len(sa.public_cells) == 2 + 601 * 4
    with pytest.raises(ValueError):
        CS.columns(sa, 14, 10, device="cpu", expose=True, break_rows=2039)
