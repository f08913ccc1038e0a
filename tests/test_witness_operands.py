"""CPU: the catalogue of structured witness steps (tests/witness_operands.py) -- what it covers, pinned, and
the reference model of the expansion (oracle/pyref.py) examined on every one of its steps, so that the GPU expectations of
tests/test_gpu_witness_structured.py do not rest on an unexamined model.  No device."""
import ctypes as C

import pytest

from oracle import pyref as P
from tests import witness_operands as WO


def test_shapes_stand_at_the_edges():
    Ls, Ws, lbs = ({s[i] for s in WO.SHAPES} for i in range(3))
    assert {2, 3, 32, 33, 64, 65, 96, 97, 128} <= Ls and {16, 17, 32, 63, 64, 65, 88, 90} <= Ws and {4, 32} <= lbs
    assert all(WO.admitted(*s) == "" for s in WO.SHAPES)
    assert all(W == 64 for L, W, _ in WO.SHAPES if L == 128)
    assert {WO.per(L) for L, _, _ in WO.SHAPES} == {1, 2, 3, 4}
    assert [WO.per(L) for L in (32, 33, 64, 65, 96, 97, 128)] == [1, 2, 2, 3, 3, 4, 4]
    # shapes per tail pattern (no tail gate, one bit, a shifted digit) of range_check(limb, W) and of range_check(carry, cb), in every class
    # of shapes: no cell is empty (the steps that run each pattern are in the census below)
    assert WO.tails() == {1: {"limb": [3, 1, 7], "carry": [1, 1, 9]}, 2: {"limb": [1, 1, 1], "carry": [1, 1, 1]},
                          3: {"limb": [1, 1, 1], "carry": [1, 1, 1]}, 4: {"limb": [1, 2, 1], "carry": [1, 1, 2]}}
    assert WO.carry_bits(33, 64) == 71 and 71 % 14 == 1
    # at W = 64 the carry has 72 bits for every L from 65 to 128, and 71 is prime: no admitted lb leaves a one-bit carry tail there, so
    # PER = 3 and PER = 4 take it from 17-bit limbs (cb = 25)
    assert {WO.carry_bits(L, 64) for L in range(65, 129)} == {72} and all(72 % lb != 1 for lb in range(4, 33))
    assert WO.carry_bits(65, 17) == WO.carry_bits(97, 17) == 25 and 25 % 8 == 25 % 4 == 1


def test_shapes_just_outside_are_refused_by_the_library():
    """pz_witness_cells_per_step is host logic: the status of every edge shape is the one make_params' documented rules give"""
    import paillier_halo2_amd as pz

    lib = pz._lib.lib()
    want = {"": 0, "unsupported": pz._lib.PZ_ERR_UNSUPPORTED, "invalid": pz._lib.PZ_ERR_INVALID}
    a, l = C.c_size_t(), C.c_size_t()
    seen = set()
    for shape in WO.EDGES + WO.SHAPES:
        st = WO.admitted(*shape)
        seen.add(st)
        assert lib.pz_witness_cells_per_step(*shape, C.byref(a), C.byref(l)) == want[st], shape
    assert seen == set(want)
    assert [WO.admitted(*s) for s in WO.EDGES] == ["unsupported"] * 4 + [""] + ["invalid"] * 5
    # the rule 2 W + ceil(log2 L) + 3 <= 192 never binds inside 16 <= W <= 90, 2 <= L <= 128
    assert max(2 * W + WO.ceil_log2(L) + 3 for W in (90,) for L in range(2, 129)) == 190


# steps of the catalogue, cut as the GPU tests cut them, that visit each class -- per class of shapes (terms per lane of the scan)
CENSUS = {
    1: {"limb>=2^128": 804, "nb=2^W": 546, "r_i=n_i|b=0": 465, "r_i=n_i|b=1": 908, "final_borrow=0": 206, "e0@0": 550, "e0@mid": 172, "e0@final": 66,
        "diff<0": 626, "diff>0": 546, "carry_top_digit": 2298, "limb_tail0": 608, "limb_tail1": 245, "limb_tail2": 1637, "carry_tail0": 219,
        "carry_tail1": 245, "carry_tail2": 2026, "slot0": 1664, "steps": 2490},
    2: {"limb>=2^128": 249, "nb=2^W": 115, "r_i=n_i|b=0": 111, "r_i=n_i|b=1": 150, "final_borrow=0": 54, "e0@0": 150, "e0@mid": 48, "e0@final": 18,
        "diff<0": 180, "diff>0": 150, "carry_top_digit": 299, "limb_tail0": 144, "limb_tail1": 144, "limb_tail2": 144, "carry_tail0": 144,
        "carry_tail1": 144, "carry_tail2": 144, "slot0": 287, "slot1": 197, "steps": 432},
    3: {"limb>=2^128": 121, "nb=2^W": 101, "r_i=n_i|b=0": 103, "r_i=n_i|b=1": 137, "final_borrow=0": 54, "e0@0": 150, "e0@mid": 48, "e0@final": 18,
        "diff<0": 180, "diff>0": 150, "carry_top_digit": 251, "limb_tail0": 144, "limb_tail1": 144, "limb_tail2": 96, "carry_tail0": 96,
        "carry_tail1": 144, "carry_tail2": 144, "slot0": 237, "slot1": 237, "slot2": 223, "steps": 384},
    4: {"limb>=2^128": 113, "nb=2^W": 69, "r_i=n_i|b=0": 80, "r_i=n_i|b=1": 92, "final_borrow=0": 72, "e0@0": 136, "e0@mid": 32, "e0@final": 24,
        "diff<0": 168, "diff>0": 104, "carry_top_digit": 226, "limb_tail0": 72, "limb_tail1": 144, "limb_tail2": 72, "carry_tail0": 72,
        "carry_tail1": 72, "carry_tail2": 144, "slot0": 198, "slot1": 137, "slot2": 180, "slot3": 140, "steps": 288},
}


def test_census_is_pinned_and_every_class_is_visited():
    got = WO.census()
    assert got == CENSUS
    for p, row in got.items():
        assert set(row) == set(WO.CENSUS) | {"slot%d" % t for t in range(p)} | {"steps"}
        assert min(row.values()) >= 1, (p, row)


def test_twelve_steps_hold_every_class():
    """the cut the largest shapes run (12 steps per modulus) visits every class under the all-ones modulus alone"""
    L, W, lb = 128, 64, 16
    n = WO.modulus("all_ones", L, W)
    tot = {}
    for s in WO.steps("all_ones", L, W, 12):
        for k, v in WO.census_of(s, n, L, W, lb).items():
            tot[k] = tot.get(k, 0) + v
    shape_only = {k for k in tot if "_tail" in k}        # one pattern per range check is the shape's, the other two are not visited
    assert min(v for k, v in tot.items() if k not in shape_only) >= 1 and len(tot) == len(WO.CENSUS) + 4, tot
    assert sorted(tot[k] for k in shape_only) == [0] * 4 + [12] * 2


def test_named_steps_are_what_their_names_say():
    L, W = 4, 64
    for odd_w in (64, 17):
        a, b = WO.final_only(L, odd_w)
        w = WO.walk(a, b, 0, 0, WO.modulus("random", L, odd_w), L, odd_w)
        assert w.e == [1] * (2 * L - 1) + [0] and w.eq == 0
    n = WO.modulus("all_ones", L, W)
    by = {s.name: s for s in WO.steps("all_ones", L, W)}
    assert (by["0*0|q=r=ones"].q, by["0*0|q=r=ones"].r) == (n, n) and by["r=n"].r == n
    w = WO.walk(*by["n-1*1"][1:5], n, L, W)
    assert w.nb[1:] == [1 << W] * (L - 1) and w.borrow == 1 and w.eq == 1      # n_i + borrow = 2^W at every limb above the first
    assert WO.walk(*by["r=n"][1:5], n, L, W).borrow == 0
    first = lambda nm: WO.walk(*by[nm][1:5], n, L, W).e.index(0)
    assert (first("r+1"), first("r+hot_mid"), first("r-hot_mid"), first("final_only")) == (0, L // 2, L // 2, 2 * L - 1)
    sign = lambda nm: [d for d in WO.walk(*by[nm][1:5], n, L, W).diffs if d][0] > 0
    assert sign("r-1") and sign("q+1") and not sign("r+1") and not sign("r+hot_mid")


def _offsets(L, W, lb):
    from paillier_halo2_amd import layout

    sc = layout.mul_mod_cells(L, W, lb)
    rc_adv, _ = layout.range_check_cells(W, lb)
    cb_adv, _ = layout.range_check_cells(WO.carry_bits(L, W), lb)
    return sc, rc_adv, cb_adv


@pytest.mark.parametrize("shape", WO.SHAPES + (WO.WIDEST,), ids=lambda s: "%d-%d-%d" % s)
def test_model_cells_on_every_catalogue_step(shape):
    """oracle/pyref.py::expand_mul_mod_cells on every step, consistent or not: it raises nothing (s >= 0: |ab_i - (qn + r)_i| <= MAX for
    operands of at most L limbs, and the carry is never negative); the gate identity a + b c = d holds on every enabled window (algebra,
    whatever walk produced the values); the limb cells recompose q, n and r; every lookup cell is below 2^lb; the last `and` cell is 1
    exactly when a b = q n + r and the last cell 1 exactly when r < n; and its carries, bits and borrows are those of the catalogue's
    own walk."""
    L, W, lb = shape
    sc, rc_adv, cb_adv = _offsets(L, W, lb)
    gates, end = P.gate_offsets_mul_mod(L, lb, W)
    assert end == sc.advice
    per_int, per_eq, per_lt, D = L + L * rc_adv, 75 + cb_adv, 11 + rc_adv, 2 * L - 1
    for name in WO.MODULI if shape != WO.WIDEST else ("all_ones",):
        n = WO.modulus(name, L, W)
        for s in WO.steps(name, L, W, WO.step_cap(L)):
            adv, lk = P.expand_mul_mod_cells(s.a, s.b, s.q, s.r, n, L, lb, W)
            assert (len(adv), len(lk)) == (sc.advice, sc.lookup)
            assert P.check_gates(adv, gates) == [], (name, s.name)
            assert max(lk) < 1 << lb
            for k, v in enumerate((s.q, n, s.r)):
                assert sum(x << (W * i) for i, x in enumerate(adv[k * per_int: k * per_int + L])) == v
            ok = s.a * s.b == s.q * n + s.r
            assert adv[sc.seg["lt"] - 1] == int(ok) and adv[-1] == int(s.r < n), (name, s.name)
            assert ok == s.honest, (name, s.name)
            w = WO.walk(s.a, s.b, s.q, s.r, n, L, W)
            eq0 = sc.seg["eq"] + 2
            assert [adv[eq0 + i * per_eq + 11] for i in range(D)] == w.carries and max(w.carries[:-1]) >> WO.carry_bits(L, W) == 0
            assert [adv[eq0 + i * per_eq + 73] for i in range(D)] + [adv[sc.seg["lt"] - 2]] == w.e
            assert adv[sc.seg["lt"] - 1] == w.eq
            assert [adv[sc.seg["lt"] + i * per_lt + 2] for i in range(L)] == w.borrow_in
            assert [adv[sc.seg["lt"] + i * per_lt + 3] for i in range(L)] == w.nb and adv[-1] == w.borrow


def test_break_point_restatements_agree():
    """the catalogue's break-point walk (with the dependency's assertion) against oracle/circuit.py's and the library's, on the masks of
    the circuits the GPU tests place, at every max_rows they use"""
    import numpy as np

    import paillier_halo2_amd as pz
    from oracle import circuit as CQ
    from paillier_halo2_amd import layout

    n = WO.circuit_keys(128)["pow2_plus1"]
    _, sg, sr, _ = P.encrypt_trace(n, n + 1, 1, n - 1)
    for kind, bits, W, lb, ng, nr in (("encrypt", 128, 64, 15, len(sg), len(sr)), ("add", 264, 88, 15, 0, 0)):
        mask, n_cells = P.gate_mask_circuit(kind, bits, W, lb, ng, nr)
        skipped = 0
        for max_rows in (8, 9, 10, 11, 64):
            want = WO.break_points(mask.tolist(), max_rows)
            if want is None:
                skipped += 1
                with pytest.raises(pz.PzError) as e:
                    layout.break_points(mask, max_rows)
                assert e.value.status == pz._lib.PZ_ERR_UNSUPPORTED
                continue
            assert want == CQ.break_points(mask, max_rows) == layout.break_points(mask, max_rows).tolist()
        assert skipped <= 1
    # a gate one cell, or two, before the gate that breaks the column: the dependency asserts it away, both walks refuse
    for back in (1, 2):
        bad = np.zeros(16, dtype=np.uint8)
        bad[[5 - back, 5]] = 1
        assert WO.break_points(bad.tolist(), 8) is None
        with pytest.raises(pz.PzError) as e:
            layout.break_points(bad, 8)
        assert e.value.status == pz._lib.PZ_ERR_UNSUPPORTED
    ok = np.zeros(16, dtype=np.uint8)
    ok[[3, 6]] = 1
    assert WO.break_points(ok.tolist(), 8) == layout.break_points(ok, 8).tolist() == [0, 6, 13, 16]
    with pytest.raises(pz.PzError):
        layout.break_points(np.zeros(16, dtype=np.uint8), 7)
