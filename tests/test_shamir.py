"""CPU: t-of-T threshold decryption with Shamir shares -- the Python dealer and Lagrange exponents against the
restatement of tests/shamir_ref.py, the scheme's algebra over every subset in Python integers, the C function pz_shamir_lagrange, and
the refusals that need no device.  Every comparison is exact."""
import ctypes as C
import itertools
import math
import random

import numpy as np
import pytest

from tests import shamir_ref as SR

SHAPES = [(1, 1), (3, 2), (5, 3), (7, 7)]


def _int(words):
    return sum(int(v) << (64 * i) for i, v in enumerate(np.asarray(words).tolist()))


def _signed(exps, neg):
    return [(-1 if s else 1) * _int(row) for row, s in zip(exps, neg.tolist())]


@pytest.fixture(scope="module")
def L():
    import paillier_halo2_amd as pz

    pz.build()
    return pz.lib()


# ------------------------------------------------------------------------------------------------------------------ the Python helpers
@pytest.mark.parametrize("T,t", SHAPES + [(16, 9)])
def test_deal_shamir_equals_the_reference(T, t):
    from paillier_halo2_amd import keys

    p, q = SR.SAFE_P, SR.SAFE_Q
    key, shares = keys.deal_shamir(p, q, T, t, rand=random.Random(0x5a00 + T).randrange)
    n, g, want_shares, mu2 = SR.deal(p, q, T, t, random.Random(0x5a00 + T).randrange)
    assert (key.n, key.g, key.mu2, key.trustees, key.threshold) == (n, g, mu2, T, t) and shares == want_shares
    assert key.v_order_proved and len(key.hs) == T and all(0 <= s < n * SR.lam_of(p, q) for s in shares)
    assert list(key.hs) == [pow(key.v, s, n * n) for s in shares]
    # the shares lie on ONE polynomial of degree below t whose constant term is theta: any t of them interpolate it
    N = n * SR.lam_of(p, q)
    ids = list(range(T - t + 1, T + 1))
    assert sum(mu * shares[i - 1] for mu, i in zip(SR.lagrange(T, ids), ids)) % N == math.factorial(T) * SR.theta_of(p, q) % N


def test_deal_shamir_with_a_general_g_and_ordinary_primes():
    from paillier_halo2_amd import keys
    from tests import decrypt_ref as DR

    p, q = DR.primes(128)
    g = DR.key(128, standard_g=False, seed=5)[1]
    key, shares = keys.deal_shamir(p, q, 5, 3, g=g, rand=random.Random(0x5a10).randrange)
    n, g2, want_shares, mu2 = SR.deal(p, q, 5, 3, random.Random(0x5a10).randrange, g=g)
    assert (key.n, key.g, key.mu2) == (n, g2, mu2) and shares == want_shares and not key.v_order_proved
    assert isinstance(key, keys.ShamirKey) and not isinstance(key, keys.ThresholdKey)


def test_deal_shamir_uses_secrets_by_default_and_refuses():
    from paillier_halo2_amd import keys

    p, q = SR.SAFE_P, SR.SAFE_Q
    (k1, s1), (k2, s2) = keys.deal_shamir(p, q, 3, 2), keys.deal_shamir(p, q, 3, 2)
    assert s1 != s2 and k1.mu2 == k2.mu2
    for T, t in ((0, 1), (257, 1), (3, 0), (3, 4), (True, 1), (3, True), (3.0, 2), (3, 2.0)):
        with pytest.raises(ValueError):
            keys.deal_shamir(p, q, T, t)
    with pytest.raises(ValueError):
        keys.deal_shamir(p, p, 3, 2)
    with pytest.raises(ValueError):                      # 5! is no unit mod 5 * 7
        keys.deal_shamir(5, 7, 5, 2)
    with pytest.raises(ValueError):
        keys.deal_shamir(p, q, 3, 2, g=p)


@pytest.mark.parametrize("T,t", SHAPES + [(16, 9), (256, 1), (256, 2), (256, 129), (256, 256)])
def test_lagrange_exponents_equal_the_reference_and_are_integers(T, t):
    from paillier_halo2_amd import keys

    rng = random.Random(0x5a20 + T + t)
    for ids in ([*range(1, t + 1)], [*range(T - t + 1, T + 1)], rng.sample(range(1, T + 1), t)):
        got = keys.lagrange_exponents(T, ids)
        assert got == SR.lagrange(T, ids) and all(isinstance(m, int) and m != 0 for m in got)    # SR.lagrange asserts integrality
        assert all(abs(m) <= math.factorial(T) ** 2 < 1 << 3368 for m in got)
    if t == 1:
        assert keys.lagrange_exponents(T, [T]) == [math.factorial(T)]
    for bad in ([], [0], [T + 1], [1, 1], [True], [1.0]):
        with pytest.raises(ValueError):
            keys.lagrange_exponents(T, bad)


@pytest.mark.parametrize("T,t", SHAPES)
def test_every_subset_recovers_m_and_one_member_fewer_fails(T, t):
    """the scheme in Python integers at a 128-bit n: every t-subset opens to m by the sign split, every (t - 1)-subset with its own
    exponents fails A = B mod n"""
    from paillier_halo2_amd import keys

    rng = random.Random(0x5a30 + T)
    key, shares = keys.deal_shamir(SR.SAFE_P, SR.SAFE_Q, T, t, rand=rng.randrange)
    n = key.n
    for m in (0, 1, n - 1, rng.randrange(n)):
        c = SR.encrypt(n, key.g, m, rng.randrange(1, n))
        us = {i: SR.partial(c, shares[i - 1], n) for i in range(1, T + 1)}
        for ids in itertools.combinations(range(1, T + 1), t):
            mus = keys.lagrange_exponents(T, ids)
            A, B = SR.split_products(mus, [us[i] for i in ids], n)
            assert A % n == B % n and A == B * (1 + (A - B) % (n * n) // n * pow(B % n, -1, n) % n * n) % (n * n)
            assert SR.combine(mus, [us[i] for i in ids], n, key.mu2) == (m, 0)
        if t > 1:
            for ids in itertools.combinations(range(1, T + 1), t - 1):
                mus = keys.lagrange_exponents(T, ids)
                assert SR.combine(mus, [us[i] for i in ids], n, key.mu2) == (0, SR.F_MISMATCH)


def test_the_reference_crt_power_is_pow():
    p, q = SR.SAFE_P, SR.SAFE_Q
    n2 = (p * q) ** 2
    rng = random.Random(0x5a38)
    for b, e in [(rng.randrange(2, n2), rng.getrandbits(256)) for _ in range(8)] + [(p, 5), (q * q, 3), (1, 0), (n2 - 1, 1), (p * q + 1, n2)]:
        assert SR.pow_n2(b, e, p, q) == pow(b, e, n2)
    c = SR.encrypt(p * q, p * q + 1, 12345, 999, pq=(p, q))
    assert c == SR.encrypt(p * q, p * q + 1, 12345, 999) and SR.partial(c, 777, p * q, pq=(p, q)) == SR.partial(c, 777, p * q)


# ------------------------------------------------------------------------------------------------------------------ the C function
def _c_lagrange(L, T, ids, cap=64):
    ids_a = np.array(ids, dtype=np.uint32)
    exps = np.zeros((max(len(ids), 1), cap), dtype=np.uint64)
    neg = np.full(max(len(ids), 1), 0xEE, dtype=np.uint8)
    need = C.c_uint32(0xFFFF)
    rc = L.pz_shamir_lagrange(T, len(ids), ids_a.ctypes.data, exps.ctypes.data, cap, neg.ctypes.data, C.byref(need))
    return rc, exps, neg, need.value


@pytest.mark.parametrize("T,t", SHAPES + [(16, 9), (256, 1), (256, 2), (256, 129), (256, 256)])
def test_c_lagrange_equals_the_python_one(L, T, t):
    from paillier_halo2_amd import keys
    from paillier_halo2_amd.engine import Engine

    rng = random.Random(0x5a40 + T + t)
    for ids in ([*range(1, t + 1)], [*range(T - t + 1, T + 1)], rng.sample(range(1, T + 1), t)):
        rc, exps, neg, need = _c_lagrange(L, T, ids)
        want = keys.lagrange_exponents(T, ids)
        assert rc == 0 and _signed(exps, neg) == want
        assert need == max(-(-abs(m).bit_length() // 64) for m in want) <= 53
        e2, n2 = Engine.shamir_lagrange(T, ids)                      # the binding trims to the longest magnitude
        assert e2.shape == (t, need) and _signed(e2, n2) == want


def test_c_lagrange_refusals_and_capacity(L):
    from paillier_halo2_amd import _lib

    inv = _lib.PZ_ERR_INVALID
    for T, ids in ((0, [1]), (257, [1]), (3, []), (3, [1, 2, 3, 1]), (3, [0]), (3, [4]), (3, [2, 2]), (256, [257])):
        assert _c_lagrange(L, T, ids)[0] == inv, (T, ids)
    ids = np.array([1, 2], dtype=np.uint32)
    buf = np.zeros(8, dtype=np.uint64)
    neg = np.zeros(2, dtype=np.uint8)
    assert L.pz_shamir_lagrange(3, 2, None, buf.ctypes.data, 4, neg.ctypes.data, None) == inv
    assert L.pz_shamir_lagrange(3, 2, ids.ctypes.data, None, 4, neg.ctypes.data, None) == inv
    assert L.pz_shamir_lagrange(3, 2, ids.ctypes.data, buf.ctypes.data, 4, None, None) == inv
    assert L.pz_shamir_lagrange(3, 2, ids.ctypes.data, buf.ctypes.data, 0, neg.ctypes.data, None) == inv
    assert L.pz_shamir_lagrange(3, 2, ids.ctypes.data, buf.ctypes.data, 4, neg.ctypes.data, None) == 0      # words_needed may be NULL
    # a short exp_words: PZ_ERR_CAPACITY, words_needed set, exps_out untouched; the exact size passes
    T, sub = 256, list(range(64, 193))
    rc, _, _, need = _c_lagrange(L, T, sub)
    assert rc == 0 and need > 1
    rc2, exps2, _, need2 = _c_lagrange(L, T, sub, cap=need - 1)
    assert rc2 == _lib.PZ_ERR_CAPACITY and need2 == need and not exps2.any()
    rc3, exps3, neg3, _ = _c_lagrange(L, T, sub, cap=need)
    from paillier_halo2_amd import keys

    assert rc3 == 0 and _signed(exps3, neg3) == keys.lagrange_exponents(T, sub)


# ------------------------------------------------------------------------------------------------------------------ refusals without a device
def test_device_entry_points_refuse_a_null_context(L):
    """the first refusal of both device entry points needs no device: a null context is PZ_ERR_INVALID (the others are in
    tests/test_gpu_shamir.py: they come after it)"""
    from paillier_halo2_amd import _lib

    a = np.ones(8, dtype=np.uint64)
    f = np.zeros(4, dtype=np.uint8)
    p = lambda x: x.ctypes.data
    for fn in (L.pz_bigint_mod_inverse, L.pz_bigint_mod_inverse_dev):
        assert fn(None, 1, 1, p(a), p(a), p(a), p(f)) == _lib.PZ_ERR_INVALID
    for fn in (L.pz_paillier_combine_t, L.pz_paillier_combine_t_dev):
        assert fn(None, 1, 1, 1, p(a), p(a), p(a), 1, p(f), p(a), p(a), p(f)) == _lib.PZ_ERR_INVALID
