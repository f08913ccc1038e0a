"""CPU: T-of-T threshold decryption (circuit kind 7 / "partial") -- the dealer's identities in Python integers,
cell totals, the gate mask and the exposed cells of the Python layers against the independent restatement of tests/partial_ref.py, the
honest stream and the five forged edges under a column-form satisfiability check, and the statement's refusals.  No device."""
import math
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import decrypt_ref as DR
from tests import partial_ref as TR

# the satisfiability shape: 128-bit n, 64-bit limbs, K = 1 -- two chains of 256 in-circuit bits, 1025 mul_mod blocks, 1.24 million
# cells.  lookup_bits 13 as the ballot's shape; k = 14 is then the smallest k (the table needs lookup_bits < k): 76 advice columns
S1P = dict(bits=128, W=64, lb=13, k=14, K=1)


def _general_g(p, q, seed):
    n = p * q
    rng = random.Random(seed)
    while True:
        a, b = rng.randrange(1, n), rng.randrange(1, n)
        if math.gcd(a, n) == 1 and math.gcd(b, n) == 1:
            return (1 + a * n) * pow(b, n, n * n) % (n * n)


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("general_g", [False, True])
@pytest.mark.parametrize("safe", [True, False])
def test_dealing_identities(T, general_g, safe):
    from paillier_halo2_amd import keys

    p, q = (TR.SAFE_P, TR.SAFE_Q) if safe else DR.primes(128)
    g = _general_g(p, q, 0x7b01 + T) if general_g else None
    rng = random.Random(0x7b02 + T)
    key, shares = keys.deal_shares(p, q, T, g=g, rand=rng.randrange)
    n, n2 = p * q, p * q * p * q
    lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    N, theta = n * lam, TR.theta_of(p, q)
    assert theta % lam == 0 and theta % n == 1 and theta < N < n2
    assert key.n == n and key.g == (n + 1 if g is None else g) and len(shares) == len(key.hs) == T
    assert all(0 <= s < N for s in shares) and (sum(shares) - theta) % N == 0
    assert key.v_order_proved is safe
    assert list(key.hs) == [pow(key.v, s, n2) for s in shares] and key.mu2 == TR.mu2_of(n, key.g, theta)
    a = (pow(key.g, theta, n2) - 1) // n
    assert math.gcd(a, n) == 1 and (a == 1) == (g is None)
    w_ok = pow(key.v, N // 2, n2) == 1            # v is a square: its order divides the exponent of the squares
    assert w_ok and key.v != 1
    if safe:
        assert all(pow(key.v, N // 2 // l, n2) != 1 for l in (p, q, (p - 1) // 2, (q - 1) // 2))
    for m in (0, 1, 12345, n - 1):
        c = P.paillier_enc_native(n, key.g, m, rng.randrange(1, n))
        us = [TR.partial(c, s, n) for s in shares]
        assert TR.combine(us, n, key.mu2) == (m, 0)
        assert pow(c, theta, n2) == (1 + a * m * n) % n2
    if T >= 2:
        c = P.paillier_enc_native(n, key.g, 7, 11)
        us = [TR.partial(c, s, n) for s in shares]
        assert TR.combine(us[:-1] + [us[0]], n, key.mu2) == (0, 1)      # a partial taken twice: the product is not 1 mod n


def test_dealing_uses_secrets_by_default_and_refuses():
    from paillier_halo2_amd import keys

    k1, s1 = keys.deal_shares(TR.SAFE_P, TR.SAFE_Q, 3)
    k2, s2 = keys.deal_shares(TR.SAFE_P, TR.SAFE_Q, 3)
    assert s1 != s2 and k1.mu2 == k2.mu2 and k1.v_order_proved and k2.v_order_proved
    p, q = DR.primes(128)
    for bad in (0, 257, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            keys.deal_shares(p, q, bad)
    assert len(keys.deal_shares(p, q, 256, rand=random.Random(1).randrange)[1]) == 256
    for pp, qq, g in ((p, p, None), (2, q, None), (p, q, 0), (p, q, (p * q) ** 2), (3, 7, None), (p, q, p)):
        with pytest.raises(ValueError):      # what secret_from_primes refuses
            keys.secret_from_primes(pp, qq, g)
        with pytest.raises(ValueError):
            keys.deal_shares(pp, qq, 2, g=g)


def _inputs(bits, K, seed):
    """n, v, an even theta with the top bit of its 2 enc_bits set, cts: integers below n^2 / 2^(2 enc_bits), as the circuit sees them"""
    rng = random.Random(seed)
    n = P.synth_paillier_inputs(bits, seed)[0]
    n2 = n * n
    v = rng.randrange(2, n2)
    theta = (1 << (2 * bits - 1)) | (rng.getrandbits(2 * bits - 1) & ~1)
    cts = [[n2 - 1, 1][i - 1] if 1 <= i < 3 else rng.randrange(2, n2) for i in range(K)]
    return n, v, theta, cts


def test_trace_and_record_order():
    bits, K, e_bits = 128, 2, 5
    n, v, _, cts = _inputs(bits, K, 0x7b10)
    n2 = n * n
    theta = 0b10110
    tr = TR.partial_trace(n, v, theta, cts, e_bits)
    recs = TR.records(tr)
    assert len(recs) == TR.n_records(K, e_bits) == K + (K + 1) * 2 * e_bits
    assert tr.h == pow(v, theta, n2) and tr.us == [pow(c * c % n2, theta, n2) for c in cts]
    assert [r[:2] for r in recs[:K]] == [(c, c) for c in cts] and [r[3] for r in recs[:K]] == [c * c % n2 for c in cts]
    for i in range(K + 1):
        ch = recs[K + i * 2 * e_bits: K + (i + 1) * 2 * e_bits]
        assert ch[0][:2] == (1, v if i == 0 else recs[i - 1][3])
        assert all(ch[2 * t + 1][0] == ch[2 * t + 1][1] == ch[2 * t][1] for t in range(e_bits))      # the step (sq, sq) follows (acc, sq)


@pytest.mark.parametrize("bits,W,lb", [(128, 64, 10), (264, 88, 11)])
@pytest.mark.parametrize("K", [1, 3])
def test_counts_gate_mask_and_public_cells_equal_the_reference(bits, W, lb, K):
    """layout and circuit_structure against the reference's stream: cell totals, segment offsets, the gate mask, the exposed cells.  The
    reference stream is expanded at the circuit's own 2 enc_bits bits."""
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    n, v, theta, cts = _inputs(bits, K, 0x7b20 + K)
    Ln = bits // W
    L = 2 * Ln
    tr = TR.partial_trace(n, v, theta, cts, 2 * bits)
    adv, lk, seg = TR.partial_cells(n, v, theta, cts, tr.h, tr.us, bits, W, lb, tr)
    assert seg["satisfied"]
    cc = layout.circuit_cells("partial", Ln, W, lb, count=K)
    assert (cc.advice, cc.lookup) == (len(adv), len(lk))
    for name in ("assign_n", "assign_v", "assign_theta", "assign_cts", "square", "refresh", "load_zero", "chains", "results", "end"):
        assert cc.seg[name] == seg[name], name
    mask = TR.partial_gate_mask(K, bits, W, lb)
    assert mask.shape[0] == len(adv)
    sa = CS.stream_structure("partial", bits, W, lb, count=K)
    assert (sa.n_cells, sa.n_steps_g, sa.n_steps_r) == (cc.advice, 2 * L * W, 0)
    assert np.array_equal(sa.gate_mask, mask)
    wide = layout.assign_cells(L, W, lb)[0]
    per = wide + layout.assert_equal_cells(L)
    res0 = cc.seg["results"][0]
    want = list(range(Ln)) + [cc.seg["assign_v"][0] + j for j in range(L)] + [res0 + j for j in range(L)]
    for i in range(K):
        want += [cc.seg["assign_cts"][0] + i * wide + j for j in range(L)] + [res0 + (i + 1) * per + j for j in range(L)]
    assert sa.public_cells.tolist() == want and len(want) == Ln + (2 + 2 * K) * L
    assert [adv[c] for c in want] == TR.statement(n, v, tr.h, cts, tr.us, bits, W)
    # the closed form: K + (K + 1) 2 E blocks, the selects, a [1, 0] pair and 2 Ln num_to_bits per chain
    mm = layout.mul_mod_cells(L, W, lb)
    E = L * W
    assert cc.seg["results"][0] - cc.seg["chains"][0] == (K + (K + 1) * 2 * E) * mm.advice + (K + 1) * (E * 8 * L + 2 + L * (7 * W - 2))


@pytest.fixture(scope="module")
def s1p():
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k, K = (S1P[f] for f in ("bits", "W", "lb", "k", "K"))
    inp = _inputs(bits, K, 0x7b30)
    sa = CS.stream_structure("partial", bits, W, lb, count=K)
    return inp, sa, CS.columns(sa, k, lb, device="cpu", expose=True)


def _placed(cs, starts, inp, trace=None, claimed=None, instances=None):
    bits, W, lb, k = (S1P[f] for f in ("bits", "W", "lb", "k"))
    n, v, theta, cts = inp
    tr = TR.partial_trace(n, v, theta, cts, 2 * bits) if trace is None else trace
    h, us = (tr.h, tr.us) if claimed is None else claimed
    adv, lk, _ = TR.partial_cells(n, v, theta, cts, h, us, bits, W, lb, tr)
    inst = TR.statement(n, v, h, cts, us, bits, W) if instances is None else instances
    return TR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, inst)


def _check(cs, cols):
    return TR.check_columns(cs.selectors, cs.map_col, cs.map_row, range(1 << S1P["lb"]), cols, cs.n_lk)


def test_honest_stream_satisfies_the_python_structure(s1p):
    from paillier_halo2_amd import layout

    inp, sa, (cs, starts) = s1p
    assert layout.break_points(sa.gate_mask, cs.max_rows).tolist() == starts[: cs.n_adv_used + 1].tolist()
    assert cs.n_instance == 1 and cs.n_adv_used >= 2                                                    # break points are crossed
    assert _check(cs, _placed(cs, starts, inp)) == []
    only_copy = lambda bad: bool(bad) and {t for t, _, _ in bad} == {"copy"}
    n, v, theta, cts = inp
    tr = TR.partial_trace(n, v, theta, cts, 2 * S1P["bits"])
    # a wrong claimed partial: only the copy of its assert_equal_fresh's bit to the constant 1 fails; the same for a wrong h
    assert only_copy(_check(cs, _placed(cs, starts, inp, claimed=(tr.h, [tr.us[0] ^ 2]))))
    assert only_copy(_check(cs, _placed(cs, starts, inp, claimed=(tr.h ^ 1, tr.us))))
    # the proof checked against another trustee's h: the statement's h differs from the witness's
    inst = TR.statement(n, v, tr.h ^ 4, cts, tr.us, S1P["bits"], S1P["W"])
    assert only_copy(_check(cs, _placed(cs, starts, inp, instances=inst)))


FORGES = [("exp", 1, None), ("base", 1), ("ct", 1, 1), ("sq", 1, 1), ("res", 0, 1)]


@pytest.mark.parametrize("forge", FORGES, ids=lambda f: f[0])
def test_forged_edges_fail(s1p, forge):
    """every forge is consistent downstream (the claimed h and u are what the forged chains give, so every gate, every lookup and every
    final equality holds): a copy constraint alone objects"""
    inp, sa, (cs, starts) = s1p
    n, v, theta, cts = inp
    if forge[0] == "exp":
        forge = ("exp", 1, theta + 1)            # chain 1 run with theta + 1 while assign_integer(theta) keeps theta
    ft = TR.partial_trace(n, v, theta, cts, 2 * S1P["bits"], forge=forge)
    honest = TR.partial_trace(n, v, theta, cts, 2 * S1P["bits"])
    assert (ft.h, ft.us) != (honest.h, honest.us)
    bad = _check(cs, _placed(cs, starts, inp, trace=ft))
    assert bad and {t for t, _, _ in bad} == {"copy"}


def test_statement_order_and_refusals():
    from paillier_halo2_amd import verifier as PV

    bits, W, K = 128, 64, 3
    Ln = bits // W
    n, v, theta, cts = _inputs(bits, K, 0x7b40)
    n2 = n * n
    h = pow(v, theta, n2)
    us = [pow(c * c % n2, theta, n2) for c in cts]
    kw = dict(enc_bits=bits, limb_bits=W)
    st = PV.public_inputs("partial", n=n, v=v, h=h, cts=cts, partials=us, **kw)
    assert st == TR.statement(n, v, h, cts, us, bits, W) and len(st) == Ln + (2 + 2 * K) * 2 * Ln
    ok = dict(v=v, h=h, cts=cts, partials=us)
    for bad in (dict(v=n2), dict(h=n2), dict(cts=[n2] + cts[1:]), dict(partials=us[:-1] + [n2 + 5]),      # >= n^2
                dict(partials=us[:-1]), dict(cts=cts[:-1]), dict(cts=[], partials=[]),                   # lengths
                dict(v=None), dict(h=None), dict(cts=None), dict(partials=None),
                dict(v=-1), dict(g=n + 1), dict(c=us[0]), dict(m=1), dict(total=1), dict(weights=[1, 1, 1])):
        with pytest.raises(ValueError):
            PV.public_inputs("partial", n=n, **{**ok, **bad}, **kw)
    for kind in ("encrypt", "decrypt", "ballot", "tally"):
        with pytest.raises(ValueError):
            PV.public_inputs(kind, n, n + 1, us[0], v=v, **kw)


def test_argument_refusals():
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    for K in (None, 0, 1025):
        with pytest.raises(ValueError):
            layout.circuit_cells("partial", 2, 64, 10, count=K)
        with pytest.raises(ValueError):
            CS.stream_structure("partial", 128, 64, 10, count=K)
    with pytest.raises(ValueError):
        layout.circuit_cells("partial", 2, 64, 10, count=1, n_steps_r=1)
    with pytest.raises(ValueError):
        layout.circuit_cells("partial", 2, 64, 10, count=1, w_bits=1)
    with pytest.raises(ValueError):
        layout.circuit_cells("partial", 2, 64, 10, count=1, m_bits=1)
    with pytest.raises(ValueError):
        CS.stream_structure("partial", 128, 64, 10, count=1, m_bits=1)
    with pytest.raises(ValueError):
        CS.stream_structure("encrypt", 128, 64, 10, exp_g=1, exp_r=3, count=1)
