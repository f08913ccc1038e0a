"""CPU: the packed ballot (kind 11 / "pballot") -- the scheme in Python integers (packing, the homomorphic
tally slot by slot, the capacity bound), cell totals and segment offsets against the reference stream, the statement's order and
refusals, the block-count arithmetic, and the Python structure generator held against the independent restatement of
tests/pballot_ref.py by a column-form satisfiability check, with the forged edges.  No device."""
import math
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import pballot_ref as PR

# R = 2 ciphertexts of K = 2 one-bit slots: 2 (4 + 128 + 2) = 268 blocks
P1S = dict(bits=128, W=64, lb=10, k=13, R=2, K=2, b=1, w=8, sl=1)


def _unit(rng, n):
    while True:
        x = rng.randrange(2, n)
        if math.gcd(x, n) == 1:
            return x


def _inputs(bits, Rn, K, b, w, s_bits, seed):
    """-> (n, g, hs, gs, vs, ss): values 0, 2^b - 1, a lone top bit, then random; the s_i likewise"""
    rng = random.Random(seed)
    n, g = P.synth_paillier_inputs(bits, seed)[:2]
    hs = PR.djn_hs(n, _unit(rng, n))
    special_v = [0, (1 << b) - 1, 1 << (b - 1)]
    special_s = [(1 << s_bits) - 1, 1 << (s_bits - 1), 0]
    flat = [special_v[i] if i < 3 else rng.randrange(1 << b) for i in range(Rn * K)]
    vs = [flat[i * K:(i + 1) * K] for i in range(Rn)]
    ss = [special_s[i] if i < 3 else rng.randrange(1 << s_bits) for i in range(Rn)]
    return n, g, hs, PR.bases(n, g, K, w), vs, ss


def test_packed_ciphertext_decrypts_to_the_packed_plaintext():
    from paillier_halo2_amd import keys

    p, q = PR.SAFE_P, PR.SAFE_Q
    n = p * q
    n2, g = n * n, n + 1
    rng = random.Random(0xb011)
    hs = PR.djn_hs(n, _unit(rng, n))
    K, w, b, s_bits = 5, 12, 3, 40
    gs = PR.bases(n, g, K, w)
    assert gs[0] == g and all(gs[j] == pow(gs[j - 1], 1 << w, n2) for j in range(1, K))
    for values in ([0] * K, [(1 << b) - 1] * K, [1 << (b - 1), 0, 7, 0, 1], [rng.randrange(1 << b) for _ in range(K)]):
        s = rng.randrange(1 << s_bits)
        tr = PR.pballot_trace(n, hs, gs, [values], [s], b, s_bits)
        c = tr.cts[0]
        assert c == PR.encrypt(n, g, hs, values, w, s)                        # (prod G_j^v_j) hs^s == g^M hs^s
        M = PR.decrypt(p, q, g, c)[0]
        assert M == sum(v << (j * w) for j, v in enumerate(values)) == keys.pack_choices(values, w)
        assert keys.unpack_tally(M, K, w) == values == PR.unpack(M, K, w)
        assert len(PR.records(tr)) == PR.per_entry(K, b, s_bits)


def test_product_of_packed_ballots_unpacks_to_the_slot_sums_and_the_capacity_is_tight():
    from paillier_halo2_amd import keys

    p, q = PR.SAFE_P, PR.SAFE_Q
    n = p * q
    n2, g = n * n, n + 1
    rng = random.Random(0xb012)
    hs = PR.djn_hs(n, _unit(rng, n))
    K, w, b = 4, 5, 2
    cap = keys.pballot_capacity(w, b)
    assert cap == PR.capacity(w, b) == 31 // 3 == 10
    assert keys.pballot_capacity(8, 1) == 255 and keys.pballot_capacity(3, 3) == 1 and keys.pballot_capacity(64, 64) == 1

    def tally(ballots):
        prod = 1
        for values in ballots:
            prod = prod * PR.encrypt(n, g, hs, values, w, rng.randrange(1 << 32)) % n2
        return PR.decrypt(p, q, g, prod)[0]

    # V random ballots within the capacity: the per-slot sums
    V = 7
    ballots = [[rng.randrange(1 << b) for _ in range(K)] for _ in range(V)]
    assert keys.unpack_tally(tally(ballots), K, w) == [sum(bl[j] for bl in ballots) for j in range(K)]
    # the bound is tight: cap ballots of the greatest value in slot 1 still stand in slot 1 alone ...
    top = [0, (1 << b) - 1, 0, 0]
    full = keys.unpack_tally(tally([top] * cap), K, w)
    assert full == [0, cap * ((1 << b) - 1), 0, 0] and full[1] < (1 << w)
    # ... and one more carries into slot 2
    over = keys.unpack_tally(tally([top] * (cap + 1)), K, w)
    assert over[2] == 1 and over[1] == (cap + 1) * ((1 << b) - 1) - (1 << w) and over != [0, (cap + 1) * ((1 << b) - 1), 0, 0]


def test_packing_helpers_refuse():
    from paillier_halo2_amd import keys

    for bad in (([], 4), ([16], 4), ([-1], 4), ([1], 0), ([True], 4)):
        with pytest.raises(ValueError):
            keys.pack_choices(*bad)
    for bad in ((1 << 8, 2, 4), (-1, 2, 4), (1, 0, 4), (1, 2, 0)):
        with pytest.raises(ValueError):
            keys.unpack_tally(*bad)
    for bad in ((4, 5), (0, 0), (4, 0)):
        with pytest.raises(ValueError):
            keys.pballot_capacity(*bad)
    # pballot_bases refuses before it asks for a device: 2^(K w) > n, no modulus, g out of range
    n = PR.SAFE_P * PR.SAFE_Q
    for bad in ((n, n + 1, 16, 8), (n, n + 1, 1, 128), (14, 3, 1, 1), (n, 0, 2, 8), (n, n * n, 2, 8), (n, n + 1, 0, 8)):
        with pytest.raises(ValueError):
            keys.pballot_bases(None, *bad)
    assert keys.pballot_bases(None, n, n + 1, 1, 127) == [n + 1]       # one slot: G_0 = g, no trace


def test_block_count_arithmetic():
    """the issue's figures: 2 b K + 2 s_bits + K blocks an entry against K (2 b + 2 s_bits + 1)"""
    per = PR.per_entry
    assert per(8, 1, 448) == 920 and 8 * per(1, 1, 448) == 7192 and per(1, 1, 448) == 899
    assert 2 * per(3, 2, 128) == 542                                       # PB1
    for K, b, s_bits in ((1, 1, 1), (64, 1, 64), (3, 2, 128), (10, 1, 65), (5, 3, 88)):
        assert per(K, b, s_bits) == 2 * b * K + 2 * s_bits + K
        assert per(1, b, s_bits) == 2 * b + 2 * s_bits + 1                # K = 1: the short-randomness ballot's entry


@pytest.mark.parametrize("bits,W,lb", [(128, 64, 10), (264, 88, 11)])
@pytest.mark.parametrize("Rn,K,b,sl", [(1, 1, 1, 1), (2, 3, 2, 1), (1, 2, 1, 2)])
def test_layout_counts_and_offsets_equal_the_reference_stream(bits, W, lb, Rn, K, b, sl):
    from paillier_halo2_amd import layout

    s_bits = sl * W
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, K, b, 8, s_bits, 0xb021 + 16 * K + b)
    tr = PR.pballot_trace(n, hs, gs, vs, ss, b, s_bits)
    assert tr.cts == [PR.encrypt(n, g, hs, row, 8, s) for row, s in zip(vs, ss)]
    adv, lk, seg = PR.pballot_cells(n, hs, gs, vs, ss, tr.cts, b, sl, bits, W, lb)
    Ln = bits // W
    cc = layout.circuit_cells("pballot", Ln, W, lb, count=Rn, slots=K, m_bits=b, s_limbs=sl)
    assert (cc.advice, cc.lookup) == (len(adv), len(lk)) and seg["satisfied"]
    names = ["assign_n", "assign_hs", "assign_bases", "values", "assign_ss", "square", "refresh", "load_zero", "entries", "results", "end"]
    for name in names + (["sums"] if K >= 2 else []):
        assert cc.seg[name] == seg[name], name
    assert ("sums" in cc.seg) == ("sums" in seg) == (K >= 2)
    assert PR.pballot_gate_mask(Rn, K, b, sl, bits, W, lb).shape[0] == len(adv)
    # the closed form of one entry: 2 b K + 2 s_bits + K blocks, the select cells, K + 1 [1, 0] pairs and the num_to_bits blocks
    mm = layout.mul_mod_cells(2 * Ln, W, lb)
    per = PR.per_entry(K, b, s_bits)
    assert cc.seg["results"][0] - cc.seg["entries"][0] == Rn * (per * mm.advice + (K * b + s_bits) * 16 * Ln + 2 * (K + 1) + K * (7 * b - 2)
                                                                + sl * (7 * W - 2))
    assert cc.seg["results"][1] - cc.seg["entries"][1] == Rn * per * mm.lookup
    # the native cell counts are host logic: no device
    from paillier_halo2_amd import _lib
    import ctypes as C

    a, l = C.c_size_t(), C.c_size_t()
    assert _lib.lib().pz_pballot_cells(Ln, W, lb, Rn, K, b, sl, C.byref(a), C.byref(l)) == 0
    assert (a.value, l.value) == (len(adv), len(lk))


@pytest.mark.parametrize("bits,W,lb,Rn,K,b,sl", [(128, 64, 10, 1, 1, 1, 1), (128, 64, 10, 2, 3, 2, 2), (264, 88, 11, 1, 2, 1, 1)])
def test_python_structure_gate_mask_and_public_cells(bits, W, lb, Rn, K, b, sl):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    s_bits = sl * W
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, K, b, 8, s_bits, 0xb031 + K)
    sa = CS.stream_structure("pballot", bits, W, lb, count=Rn, slots=K, m_bits=b, s_limbs=sl)
    assert np.array_equal(sa.gate_mask, PR.pballot_gate_mask(Rn, K, b, sl, bits, W, lb))
    Ln = bits // W
    cc = layout.circuit_cells("pballot", Ln, W, lb, count=Rn, slots=K, m_bits=b, s_limbs=sl)
    assert (sa.n_cells, sa.n_steps_g, sa.n_steps_r) == (cc.advice, 2 * b, 2 * s_bits)
    wide = layout.assign_cells(2 * Ln, W, lb)[0]
    per = wide + layout.assert_equal_cells(2 * Ln)
    want = list(range(Ln)) + [cc.seg["assign_hs"][0] + j for j in range(2 * Ln)] + \
        [cc.seg["assign_bases"][0] + t * wide + j for t in range(K) for j in range(2 * Ln)] + \
        [cc.seg["results"][0] + i * per + j for i in range(Rn) for j in range(2 * Ln)]
    if K >= 2:
        want += [cc.seg["sums"][0] + (i + 1) * (1 + 3 * (K - 1)) - 1 for i in range(Rn)]     # the last cell of each sum
        assert want[-1] == cc.seg["assign_ss"][0] - 1
    assert sa.public_cells.tolist() == want and len(want) == Ln + 2 * Ln * (1 + K + Rn) + (K >= 2) * Rn
    # ... and those cells hold the statement in the reference stream
    tr = PR.pballot_trace(n, hs, gs, vs, ss, b, s_bits)
    adv, _, _ = PR.pballot_cells(n, hs, gs, vs, ss, tr.cts, b, sl, bits, W, lb)
    assert [adv[c] for c in want] == PR.statement(n, hs, gs, tr.cts, [sum(r) for r in vs] if K >= 2 else None, bits, W)
    # the native statement cells are host logic: no device
    from paillier_halo2_amd import _lib
    import ctypes as C

    out = np.zeros(len(want) + 4, dtype=np.uint64)
    npub = C.c_size_t()
    assert _lib.lib().pz_pballot_public_cells(Ln, W, lb, Rn, K, b, sl, C.c_void_p(out.ctypes.data), out.shape[0], C.byref(npub)) == 0
    assert out[: npub.value].tolist() == want


@pytest.fixture(scope="module")
def p1s_columns():
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k, Rn, K, b, w, sl = (P1S[f] for f in ("bits", "W", "lb", "k", "R", "K", "b", "w", "sl"))
    inp = _inputs(bits, Rn, K, b, w, sl * W, 0xb041)
    sa = CS.stream_structure("pballot", bits, W, lb, count=Rn, slots=K, m_bits=b, s_limbs=sl)
    return inp, sa, CS.columns(sa, k, lb, device="cpu", expose=True), CS.columns(sa, k, lb, device="cpu")


def _placed(cs, starts, inp, trace=None, expose=True, res=None, instances=None):
    bits, W, lb, k, b, sl = (P1S[f] for f in ("bits", "W", "lb", "k", "b", "sl"))
    n, g, hs, gs, vs, ss = inp
    tr = PR.pballot_trace(n, hs, gs, vs, ss, b, sl * W) if trace is None else trace
    res = tr.cts if res is None else res
    adv, lk, _ = PR.pballot_cells(n, hs, gs, vs, ss, res, b, sl, bits, W, lb, tr)
    inst = None
    if expose:
        inst = PR.statement(n, hs, gs, res, tr.totals, bits, W) if instances is None else instances
    return PR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, inst)


def test_reference_stream_satisfies_the_python_structure(p1s_columns):
    from paillier_halo2_amd import layout

    inp, sa, (cs, starts), (cs0, starts0) = p1s_columns
    lb = P1S["lb"]
    assert inp[4] == [[0, 1], [1, inp[4][1][1]]]
    assert layout.break_points(sa.gate_mask, cs.max_rows).tolist() == starts[: cs.n_adv_used + 1].tolist()
    assert cs.n_instance == 1 and cs0.n_instance == 0 and cs.m == cs0.m + 1 and cs.n_adv_used >= 2     # break points are crossed
    table = range(1 << lb)
    check = lambda cols, c=cs: PR.check_columns(c.selectors, c.map_col, c.map_row, table, cols, c.n_lk)
    assert check(_placed(cs, starts, inp)) == []
    assert check(_placed(cs0, starts0, inp, expose=False), cs0) == []                                  # ... and without the instance column
    # an election under ANOTHER key (n, g, hs) and ANOTHER slot width on the SAME structure: neither shapes it
    n2_, g2_, hs2_, gs2_, _, _ = _inputs(P1S["bits"], P1S["R"], P1S["K"], P1S["b"], 21, P1S["sl"] * P1S["W"], 0xb042)
    assert n2_ != inp[0] and hs2_ != inp[2] and gs2_[1] == pow(g2_, 1 << 21, n2_ * n2_)
    assert check(_placed(cs, starts, (n2_, g2_, hs2_, gs2_, [[1, 1], [0, 0]], [5, (1 << 64) - 2]))) == []
    only_copy = lambda bad: bool(bad) and {t for t, _, _ in bad} == {"copy"}
    # a wrong claimed ciphertext: only the copy of its assert_equal_fresh's bit to the constant 1 fails
    n, g, hs, gs, vs, ss = inp
    tr = PR.pballot_trace(n, hs, gs, vs, ss, P1S["b"], P1S["sl"] * P1S["W"])
    assert only_copy(check(_placed(cs, starts, inp, res=[tr.cts[0], tr.cts[1] ^ 2])))
    # a statement total changed by one, a statement hs changed by one, a statement base changed by one
    st = lambda **kw: PR.statement(kw.get("n", n), kw.get("hs", hs), kw.get("gs", gs), tr.cts, kw.get("totals", tr.totals), P1S["bits"], P1S["W"])
    assert only_copy(check(_placed(cs, starts, inp, instances=st(totals=[tr.totals[0], tr.totals[1] + 1]))))
    assert only_copy(check(_placed(cs, starts, inp, instances=st(hs=hs ^ 1))))
    assert only_copy(check(_placed(cs, starts, inp, instances=st(gs=[gs[0], gs[1] ^ 1]))))


FORGES = [("val", 1, 0, 0), ("base", 0, 1, 1), ("swap", 1), ("fold", 0, 0, 1), ("fold", 1, 1, 1), ("s", 1, 6), ("sum", 0, 1)]


@pytest.mark.parametrize("forge", FORGES, ids=lambda f: "-".join(str(x) for x in f[:3]))
def test_forged_edges_fail(p1s_columns, forge):
    """every forge is consistent downstream: the claimed ciphertexts are what the forged chains give"""
    inp, sa, (cs, starts), _ = p1s_columns
    n, g, hs, gs, vs, ss = inp
    b, s_bits = P1S["b"], P1S["sl"] * P1S["W"]
    honest = PR.pballot_trace(n, hs, gs, vs, ss, b, s_bits)
    ft = PR.pballot_trace(n, hs, gs, vs, ss, b, s_bits, forge=forge)
    assert (ft.cts != honest.cts) == (forge[0] != "sum") and (ft.totals != honest.totals) == (forge[0] == "sum")
    bad = PR.check_columns(cs.selectors, cs.map_col, cs.map_row, range(1 << P1S["lb"]), _placed(cs, starts, inp, trace=ft), cs.n_lk)
    kinds = {t for t, _, _ in bad}
    assert kinds == ({"gate"} if forge[0] == "sum" else {"copy"})       # the sum's own gate objects; elsewhere a copy constraint


def test_statement_order_and_refusals():
    from paillier_halo2_amd import verifier as PV

    bits, W, Rn, K, b, w, s_bits = 128, 64, 2, 3, 2, 8, 64
    Ln = bits // W
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, K, b, w, s_bits, 0xb051)
    tr = PR.pballot_trace(n, hs, gs, vs, ss, b, s_bits)
    totals = [sum(r) for r in vs]
    kw = dict(enc_bits=bits, limb_bits=W)
    sh = dict(slots=K, slot_bits=w, m_bits=b)
    st = PV.public_inputs("pballot", n=n, g=g, hs=hs, cts=tr.cts, totals=totals, **sh, **kw)
    assert st == PR.statement(n, hs, gs, tr.cts, totals, bits, W)
    assert len(st) == Ln + 2 * Ln * (1 + K + Rn) + Rn and st[-Rn:] == totals
    # one slot: G_0 = g and no totals
    tr1 = PR.pballot_trace(n, hs, [g], [[1], [0]], ss, b, s_bits)
    one = PV.public_inputs("pballot", n=n, g=g, hs=hs, cts=tr1.cts, slots=1, slot_bits=w, m_bits=b, **kw)
    assert one == PR.statement(n, hs, [g], tr1.cts, None, bits, W) and len(one) == Ln + 2 * Ln * (1 + 1 + Rn)
    ok = dict(hs=hs, cts=tr.cts, totals=totals, **sh)
    for change in (dict(slots=16, slot_bits=8),                        # 2^(K w) = 2^128 > n
                   dict(slots=2, slot_bits=64, totals=totals),         # the same bound
                   dict(m_bits=9),                                     # m_bits > slot_bits: a value would reach into the next slot
                   dict(hs=0),                                         # every ciphertext would be 0
                   dict(hs=n * n),
                   dict(cts=[n * n, tr.cts[1]]),                       # c >= n^2
                   dict(totals=None),                                  # totals missing with K >= 2
                   dict(totals=totals[:1]),                            # a wrong length
                   dict(totals=totals + [0]),
                   dict(totals=[-1, 0]),
                   dict(slots=1),                                      # totals with K = 1 would expose the value
                   dict(slots=None), dict(slot_bits=None), dict(m_bits=None), dict(slots=0), dict(slot_bits=0), dict(m_bits=0),
                   dict(hs=None), dict(cts=[]), dict(cts=None),
                   dict(c=tr.cts[0]),                                  # no single result
                   dict(total=1),                                      # `total` is the unpacked ballots'
                   dict(m=1), dict(weights=[1, 1]), dict(mixed=tr.cts)):
        with pytest.raises(ValueError):
            PV.public_inputs("pballot", n=n, g=g, **{**ok, **change}, **kw)
    with pytest.raises(ValueError):
        PV.public_inputs("pballot", n=n, g=None, **ok, **kw)
    # slots, slot_bits, m_bits and totals belong to this kind alone
    for extra in (dict(slots=2), dict(slot_bits=8), dict(m_bits=1), dict(totals=[1])):
        with pytest.raises(ValueError):
            PV.public_inputs("sballot", n=n, g=g, hs=hs, cts=tr.cts, total=1, **extra, **kw)


def test_argument_refusals():
    import ctypes as C

    from paillier_halo2_amd import _lib
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    bad_shapes = ((None, 2, 1, 1), (0, 2, 1, 1), (1025, 1, 1, 1), (2, None, 1, 1), (2, 0, 1, 1), (2, 65, 1, 1), (17, 64, 1, 1), (513, 2, 1, 1),
                  (2, 2, None, 1), (2, 2, 0, 1), (2, 2, 65, 1), (2, 2, 1, None), (2, 2, 1, 0), (2, 2, 1, 5))
    for Rn, K, b, sl in bad_shapes:
        with pytest.raises(ValueError):
            layout.circuit_cells("pballot", 2, 64, 10, count=Rn, slots=K, m_bits=b, s_limbs=sl)
        with pytest.raises(ValueError):
            CS.stream_structure("pballot", 128, 64, 10, count=Rn, slots=K, m_bits=b, s_limbs=sl)
    with pytest.raises(ValueError):
        layout.circuit_cells("pballot", 2, 64, 10, n_steps_g=3, count=2, slots=2, m_bits=1, s_limbs=1)
    for kind, extra in (("sballot", dict(count=2, m_bits=1, s_limbs=1)), ("tally", dict(count=3)), ("add", {})):
        with pytest.raises(ValueError):
            layout.circuit_cells(kind, 2, 64, 10, slots=2, **extra)
    with pytest.raises(ValueError):
        CS.stream_structure("sballot", 128, 64, 10, count=2, m_bits=1, s_limbs=1, slots=2)
    # the C ABI's counts: host logic, PZ_ERR_INVALID = -1 for a shape out of range
    L = _lib.lib()
    a, l = C.c_size_t(), C.c_size_t()
    for Rn, K, b, sl in bad_shapes:
        if None not in (Rn, K, b, sl):
            assert L.pz_pballot_cells(2, 64, 10, Rn, K, b, sl, C.byref(a), C.byref(l)) == -1
    assert L.pz_pballot_cells(2, 64, 10, 16, 64, 1, 4, C.byref(a), C.byref(l)) == 0
    # the by-kind entry points keep refusing kind > 5
    assert L.pz_circuit_cells(11, 2, 64, 10, 0, 0, C.byref(a), C.byref(l)) == -1
    npub = C.c_size_t()
    assert L.pz_circuit_public_cells(11, 2, 64, 10, 0, 0, None, 0, C.byref(npub)) == -1
    # the K3 entry point's refusals that come before the context is looked at: a null pointer
    assert L.pz_paillier_pballot(None, 2, 1, 1, 1, 1, None, None, None, None, None, None, 0, None) == -1
