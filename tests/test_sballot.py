"""CPU: the short-randomness ballot (kind 9 / "sballot") -- the scheme in Python integers, cell totals and
segment offsets against the reference stream, the statement's order and refusals, and the Python structure generator held against the
independent restatement of tests/sballot_ref.py by a column-form satisfiability check, with the six forged edges.  No device."""
import math
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import sballot_ref as SR

S1S = dict(bits=128, W=64, lb=10, k=13, K=2, b=1, sl=1)


def _prime_3mod4(start: int) -> int:
    from paillier_halo2_amd import keys

    x = start - start % 4 + 3
    while not keys._is_prime(x):
        x += 4
    return x


def _key(bits: int):
    if bits == 128:
        return SR.SAFE_P, SR.SAFE_Q
    assert bits == 264
    return _prime_3mod4((3 << 130) + 12345), _prime_3mod4((3 << 130) + (1 << 100))


def _unit(rng, n):
    while True:
        x = rng.randrange(2, n)
        if math.gcd(x, n) == 1:
            return x


def _inputs(bits, K, b, s_bits, seed):
    rng = random.Random(seed)
    n, g = P.synth_paillier_inputs(bits, seed)[:2]
    hs = SR.djn_hs(n, _unit(rng, n))
    special_m = [0, (1 << b) - 1, 1 << (b - 1)]                   # zero, all ones, a lone top bit
    special_s = [0, (1 << s_bits) - 1, 1 << (s_bits - 1)]
    ms = [special_m[i] if i < 3 else rng.randrange(1 << b) for i in range(K)]
    ss = [special_s[(i + 1) % 3] if i < 3 else rng.randrange(1 << s_bits) for i in range(K)]
    return n, g, hs, ms, ss


@pytest.mark.parametrize("bits", [128, 264])
def test_scheme_decrypts_and_recovers_h_to_the_s(bits):
    p, q = _key(bits)
    assert p % 4 == q % 4 == 3 and p != q
    n = p * q
    assert n.bit_length() == bits
    n2, g = n * n, n + 1
    rng = random.Random(0x5b01 + bits)
    x = _unit(rng, n)
    h, hs = SR.djn_h(n, x), SR.djn_hs(n, x)
    assert hs == pow(h, n, n2) and SR.decrypt(p, q, g, hs)[0] == 0           # hs is itself an encryption of 0
    s_bits = 40
    ms = [0, 1, (1 << 16) - 1, rng.randrange(1 << 16)]
    ss = [0, (1 << s_bits) - 1, 1 << (s_bits - 1), rng.randrange(1 << s_bits)]
    cts = [SR.encrypt(n, g, hs, m, s) for m, s in zip(ms, ss)]
    for m, s, c in zip(ms, ss, cts):
        got_m, got_r = SR.decrypt(p, q, g, c)
        assert got_m == m and got_r == pow(h, s, n)                           # an ordinary ciphertext with r = h^s mod n
        assert c == pow(g, m, n2) * pow(got_r, n, n2) % n2
    prod = 1
    for c in cts:
        prod = prod * c % n2
    assert SR.decrypt(p, q, g, prod)[0] == sum(ms)
    # the trace's ciphertexts are the scheme's
    tr = SR.sballot_trace(n, g, hs, ms, ss, 16, s_bits)
    assert tr.cts == cts and len(SR.records(tr)) == len(ms) * SR.per_entry(16, s_bits)


@pytest.mark.parametrize("bits,W,lb", [(128, 64, 10), (264, 88, 11)])
@pytest.mark.parametrize("K,b,sl", [(1, 1, 1), (2, 2, 1), (3, 1, 2)])
def test_layout_counts_and_offsets_equal_the_reference_stream(bits, W, lb, K, b, sl):
    from paillier_halo2_amd import layout

    if bits == 264 and sl == 2:
        K = 2                                                                # (the reference stream in Python: keep the wide case small)
    s_bits = sl * W
    n, g, hs, ms, ss = _inputs(bits, K, b, s_bits, 0x5b11 + 16 * K + b)
    tr = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits)
    n2 = n * n
    assert tr.cts == [pow(g, m, n2) * pow(hs, s, n2) % n2 for m, s in zip(ms, ss)]
    adv, lk, seg = SR.sballot_cells(n, g, hs, ms, ss, tr.cts, b, sl, bits, W, lb)
    Ln = bits // W
    cc = layout.circuit_cells("sballot", Ln, W, lb, count=K, m_bits=b, s_limbs=sl)
    assert (cc.advice, cc.lookup) == (len(adv), len(lk)) and seg["satisfied"]
    names = ["assign_n", "assign_g", "assign_hs", "messages", "assign_ss", "square", "refresh", "load_zero", "entries", "results", "end"]
    for name in names + (["sum"] if K >= 2 else []):
        assert cc.seg[name] == seg[name], name
    assert ("sum" in cc.seg) == ("sum" in seg) == (K >= 2)
    assert SR.sballot_gate_mask(K, b, sl, bits, W, lb).shape[0] == len(adv)
    # the closed form of one entry: 2 b + 2 s_bits + 1 blocks, the select cells, two [1, 0] pairs and the num_to_bits blocks
    mm = layout.mul_mod_cells(2 * Ln, W, lb)
    per = SR.per_entry(b, s_bits)
    assert cc.seg["results"][0] - cc.seg["entries"][0] == K * (per * mm.advice + (b + s_bits) * 16 * Ln + 4 + 7 * b - 2 + sl * (7 * W - 2))
    # the native cell counts are host logic: no device
    from paillier_halo2_amd import _lib
    import ctypes as C

    a, l = C.c_size_t(), C.c_size_t()
    assert _lib.lib().pz_sballot_cells(Ln, W, lb, K, b, sl, C.byref(a), C.byref(l)) == 0
    assert (a.value, l.value) == (len(adv), len(lk))


@pytest.mark.parametrize("bits,W,lb,K,b,sl", [(128, 64, 10, 1, 1, 1), (128, 64, 10, 3, 2, 2), (264, 88, 11, 2, 1, 1)])
def test_python_structure_gate_mask_and_public_cells(bits, W, lb, K, b, sl):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    s_bits = sl * W
    n, g, hs, ms, ss = _inputs(bits, K, b, s_bits, 0x5b21 + K)
    sa = CS.stream_structure("sballot", bits, W, lb, count=K, m_bits=b, s_limbs=sl)
    assert np.array_equal(sa.gate_mask, SR.sballot_gate_mask(K, b, sl, bits, W, lb))
    Ln = bits // W
    cc = layout.circuit_cells("sballot", Ln, W, lb, count=K, m_bits=b, s_limbs=sl)
    assert (sa.n_cells, sa.n_steps_g, sa.n_steps_r) == (cc.advice, 2 * b, 2 * s_bits)
    per = layout.assign_cells(2 * Ln, W, lb)[0] + layout.assert_equal_cells(2 * Ln)
    want = list(range(Ln)) + [cc.seg["assign_g"][0] + j for j in range(Ln)] + [cc.seg["assign_hs"][0] + j for j in range(2 * Ln)] + \
        [cc.seg["results"][0] + i * per + j for i in range(K) for j in range(2 * Ln)]
    if K >= 2:
        want.append(cc.seg["assign_ss"][0] - 1)             # the last cell of the sum
    assert sa.public_cells.tolist() == want and len(want) == 2 * Ln + (K + 1) * 2 * Ln + (K >= 2)
    # ... and those cells hold the statement in the reference stream
    tr = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits)
    adv, _, _ = SR.sballot_cells(n, g, hs, ms, ss, tr.cts, b, sl, bits, W, lb)
    assert [adv[c] for c in want] == SR.statement(n, g, hs, tr.cts, sum(ms) if K >= 2 else None, bits, W)
    # the native statement cells are host logic: no device
    from paillier_halo2_amd import _lib
    import ctypes as C

    out = np.zeros(len(want) + 4, dtype=np.uint64)
    npub = C.c_size_t()
    assert _lib.lib().pz_sballot_public_cells(Ln, W, lb, K, b, sl, C.c_void_p(out.ctypes.data), out.shape[0], C.byref(npub)) == 0
    assert out[: npub.value].tolist() == want


@pytest.fixture(scope="module")
def s1s_columns():
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k, K, b, sl = (S1S[f] for f in ("bits", "W", "lb", "k", "K", "b", "sl"))
    inp = _inputs(bits, K, b, sl * W, 0x5b31)
    sa = CS.stream_structure("sballot", bits, W, lb, count=K, m_bits=b, s_limbs=sl)
    return inp, sa, CS.columns(sa, k, lb, device="cpu", expose=True), CS.columns(sa, k, lb, device="cpu")


def _placed(cs, starts, inp, trace=None, expose=True, res=None, instances=None):
    bits, W, lb, k, b, sl = (S1S[f] for f in ("bits", "W", "lb", "k", "b", "sl"))
    n, g, hs, ms, ss = inp
    tr = SR.sballot_trace(n, g, hs, ms, ss, b, sl * W) if trace is None else trace
    res = tr.cts if res is None else res
    adv, lk, _ = SR.sballot_cells(n, g, hs, ms, ss, res, b, sl, bits, W, lb, tr)
    inst = None
    if expose:
        inst = SR.statement(n, g, hs, res, tr.total, bits, W) if instances is None else instances
    return SR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, inst)


def test_reference_stream_satisfies_the_python_structure(s1s_columns):
    from paillier_halo2_amd import layout

    inp, sa, (cs, starts), (cs0, starts0) = s1s_columns
    lb = S1S["lb"]
    assert inp[3] == [0, 1]
    assert layout.break_points(sa.gate_mask, cs.max_rows).tolist() == starts[: cs.n_adv_used + 1].tolist()
    assert cs.n_instance == 1 and cs0.n_instance == 0 and cs.m == cs0.m + 1 and cs.n_adv_used >= 2     # break points are crossed
    table = range(1 << lb)
    check = lambda cols, c=cs: SR.check_columns(c.selectors, c.map_col, c.map_row, table, cols, c.n_lk)
    assert check(_placed(cs, starts, inp)) == []
    assert check(_placed(cs0, starts0, inp, expose=False), cs0) == []                                  # ... and without the instance column
    # a ballot under ANOTHER key (n, g, hs) on the SAME structure: nothing of the key but its size shapes it
    n2_, g2_, hs2_, _, _ = _inputs(S1S["bits"], S1S["K"], S1S["b"], S1S["sl"] * S1S["W"], 0x5b32)
    assert n2_ != inp[0] and hs2_ != inp[2]
    assert check(_placed(cs, starts, (n2_, g2_, hs2_, [1, 1], [5, (1 << 64) - 2]))) == []
    only_copy = lambda bad: bool(bad) and {t for t, _, _ in bad} == {"copy"}
    # a wrong claimed ciphertext: only the copy of its assert_equal_fresh's bit to the constant 1 fails
    n, g, hs, ms, ss = inp
    tr = SR.sballot_trace(n, g, hs, ms, ss, S1S["b"], S1S["sl"] * S1S["W"])
    assert only_copy(check(_placed(cs, starts, inp, res=[tr.cts[0], tr.cts[1] ^ 2])))
    # a statement total changed by one, and a statement hs changed by one
    inst = SR.statement(n, g, hs, tr.cts, tr.total + 1, S1S["bits"], S1S["W"])
    assert only_copy(check(_placed(cs, starts, inp, instances=inst)))
    inst = SR.statement(n, g, hs ^ 1, tr.cts, tr.total, S1S["bits"], S1S["W"])
    assert only_copy(check(_placed(cs, starts, inp, instances=inst)))


FORGES = [("s", 1, 6), ("base", 1, 1), ("msg", 0, 1), ("g", 1, 1), ("final", 0, 1), ("sum", 1)]


@pytest.mark.parametrize("forge", FORGES, ids=lambda f: f[0])
def test_forged_edges_fail(s1s_columns, forge):
    """every forge is consistent downstream: the claimed ciphertexts are what the forged chains give"""
    inp, sa, (cs, starts), _ = s1s_columns
    n, g, hs, ms, ss = inp
    b, s_bits = S1S["b"], S1S["sl"] * S1S["W"]
    honest = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits)
    ft = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits, forge=forge)
    assert (ft.cts != honest.cts) == (forge[0] != "sum") and (ft.total != honest.total) == (forge[0] == "sum")
    bad = SR.check_columns(cs.selectors, cs.map_col, cs.map_row, range(1 << S1S["lb"]), _placed(cs, starts, inp, trace=ft), cs.n_lk)
    kinds = {t for t, _, _ in bad}
    assert kinds == ({"gate"} if forge[0] == "sum" else {"copy"})       # the sum's own gate objects; elsewhere a copy constraint


def test_statement_order_and_refusals():
    from paillier_halo2_amd import verifier as PV

    bits, W, K, b, s_bits = 128, 64, 3, 2, 64
    Ln = bits // W
    n, g, hs, ms, ss = _inputs(bits, K, b, s_bits, 0x5b41)
    tr = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits)
    kw = dict(enc_bits=bits, limb_bits=W)
    st = PV.public_inputs("sballot", n=n, g=g, hs=hs, cts=tr.cts, total=sum(ms), **kw)
    assert st == SR.statement(n, g, hs, tr.cts, sum(ms), bits, W) and len(st) == 2 * Ln + (K + 1) * 2 * Ln + 1 and st[-1] == sum(ms)
    one = PV.public_inputs("sballot", n=n, g=g, hs=hs, cts=tr.cts[:1], **kw)
    assert one == SR.statement(n, g, hs, tr.cts[:1], None, bits, W) and len(one) == 2 * Ln + 2 * 2 * Ln
    for bad in (dict(hs=0, cts=tr.cts, total=1),                        # hs = 0: every ciphertext would be 0
                dict(hs=n * n, cts=tr.cts, total=1),                    # hs >= n^2
                dict(hs=hs, cts=[n * n] + tr.cts[1:], total=1),         # c >= n^2
                dict(hs=hs, cts=tr.cts[:1], total=ms[0]),               # a total with K = 1 would expose the message
                dict(hs=hs, cts=tr.cts),                                # a total missing with K >= 2
                dict(cts=tr.cts, total=1),                              # no hs
                dict(hs=hs, cts=[], total=None),
                dict(hs=hs, total=1),                                   # no ciphertexts
                dict(hs=hs, cts=tr.cts, total=-1),
                dict(hs=hs, cts=tr.cts, total=1, c=tr.cts[0]),          # no single result
                dict(hs=hs, cts=tr.cts, total=1, m=1),
                dict(hs=hs, cts=tr.cts, total=1, weights=[1, 1, 1])):
        with pytest.raises(ValueError):
            PV.public_inputs("sballot", n=n, g=g, **bad, **kw)
    with pytest.raises(ValueError):
        PV.public_inputs("sballot", n=n, g=None, hs=hs, cts=tr.cts, total=1, **kw)
    with pytest.raises(ValueError):
        PV.public_inputs("ballot", n=n, g=g, hs=hs, cts=tr.cts, total=1, **kw)     # hs belongs to this kind alone


def test_argument_refusals():
    import ctypes as C

    from paillier_halo2_amd import _lib
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import keys, layout

    for K, b, sl in ((None, 1, 1), (0, 1, 1), (1025, 1, 1), (2, None, 1), (2, 0, 1), (2, 65, 1), (2, 1, None), (2, 1, 0), (2, 1, 5)):
        with pytest.raises(ValueError):
            layout.circuit_cells("sballot", 2, 64, 10, count=K, m_bits=b, s_limbs=sl)
        with pytest.raises(ValueError):
            CS.stream_structure("sballot", 128, 64, 10, count=K, m_bits=b, s_limbs=sl)
    with pytest.raises(ValueError):
        layout.circuit_cells("sballot", 2, 64, 10, n_steps_g=3, count=2, m_bits=1, s_limbs=1)
    with pytest.raises(ValueError):
        layout.circuit_cells("sballot", 2, 64, 10, count=2, m_bits=1, s_limbs=1, w_bits=1)
    for kind, extra in (("ballot", dict(count=2, m_bits=1, n_steps_r=190)), ("tally", dict(count=3)), ("add", {})):
        with pytest.raises(ValueError):
            layout.circuit_cells(kind, 2, 64, 10, s_limbs=1, **extra)
    with pytest.raises(ValueError):
        CS.stream_structure("ballot", 128, 64, 10, exp_r=P.synth_paillier_inputs(128, 3)[0], count=2, m_bits=1, s_limbs=1)
    # the C ABI's counts: host logic, PZ_ERR_INVALID = -1 for a shape out of range
    L = _lib.lib()
    a, l = C.c_size_t(), C.c_size_t()
    for K, b, sl in ((0, 1, 1), (1025, 1, 1), (2, 0, 1), (2, 65, 1), (2, 1, 0), (2, 1, 5)):
        assert L.pz_sballot_cells(2, 64, 10, K, b, sl, C.byref(a), C.byref(l)) == -1
    assert L.pz_sballot_cells(2, 64, 10, 2, 1, 4, C.byref(a), C.byref(l)) == 0
    # the K3 entry point's refusals that come before the context is looked at: a null pointer
    assert L.pz_paillier_sballot(None, 2, 1, 1, 1, None, None, None, None, None, None, 0, None) == -1
    # djn_generator refuses what is no modulus before it asks for a device
    for n in (0, 4, 14, True):
        with pytest.raises(ValueError):
            keys.djn_generator(None, n)
