"""CPU: the Python-integer models of the device prime generation (tests/prime_ref.py) against each other and against keys._is_prime,
the catalogue's pinned witness indices, and keys.generate_prime / generate_key / is_probable_prime driven by a stub engine whose
prime_search and is_prime are the models."""
import math
import random

import pytest

import prime_ref as R
from paillier_halo2_amd import keys


def test_catalogue_witness_indices_are_pinned():
    assert len(R.CATALOGUE) >= 70
    for name, c, wit in R.CATALOGUE:
        flag, got = R.mr_first_witness(c, R.PRIME_BASES)
        assert got == wit, name
        assert flag == (1 if wit == R.ALL_PASS or c == 2 else 0), name
    for c, bases, wit in R.REDUCING:
        assert R.mr_first_witness(c, bases)[1] == wit, (c, bases)


def test_catalogue_agrees_with_the_fixed_base_test():
    """keys._is_prime is deterministic below 3.3e24 and runs 36 bases above: a catalogue entry passes all of PRIME_BASES iff it is prime,
    and the strong pseudoprimes are exactly the entries that pass base 2 .. and still fail"""
    for name, c, wit in R.CATALOGUE:
        assert keys._is_prime(c) == (wit == R.ALL_PASS or c == 2), name
    for name, c, wit in R.CATALOGUE[:5]:
        for k in range(wit):
            assert R.mr_first_witness(c, R.PRIME_BASES[k:k + 1]) == (1, 1), (name, k)   # each passes every earlier round
        assert R.mr_first_witness(c, R.PRIME_BASES[wit:wit + 1]) == (0, 0), name


def test_catalogue_arithmetic_facts():
    P = R.ALL_PASS
    cat = {name: (c, wit) for name, c, wit in R.CATALOGUE}
    for e, k in ((64, 59), (128, 159), (256, 189), (512, 569), (1024, 105), (2048, 1557)):
        c = 2 ** e - k
        assert cat["2^%d-%d" % (e, k)] == (c, P) and c.bit_length() == e
        assert all(not keys._is_prime(x) for x in range(c + 2, 2 ** e, 2)), "the largest prime below 2^%d" % e
    for e in (61, 89, 107, 127, 521, 607, 1279):
        assert cat["M%d" % e] == (2 ** e - 1, P)
    for k, s in ((9, 63), (25, 64), (9, 65), (205, 130), (13, 1000)):
        c = k * 2 ** s + 1
        assert cat["%d*2^%d+1" % (k, s)] == (c, P) and ((c - 1) & -(c - 1)).bit_length() - 1 == s
    for bits, (p, q) in R.golden_primes().items():
        if bits <= 2048:
            assert cat["golden n %d" % bits] == (p * q, 0) and cat["golden p^2 %d" % bits] == (p * p, 0)


def test_sieve_model_against_trial_division():
    rng = random.Random(11)
    for bits, safe, window in ((40, False, 300), (64, True, 300), (128, False, 200), (128, True, 200)):
        stride = R.stride_of(safe)
        start = (rng.getrandbits(bits) | (3 << (bits - 2))) // stride * stride + (3 if safe else 1)
        mask = R.sieve_mask(start, window, safe)
        for i in range(window):
            c = start + stride * i
            ok = all(c % p for p in R.SIEVE_PRIMES) and (not safe or all(((c - 1) // 2) % p for p in R.SIEVE_PRIMES))
            assert mask[i] == ok, (bits, safe, i)


def test_search_model_finds_what_is_prime():
    rng = random.Random(12)
    for bits, safe, window in ((64, False, 4096), (64, True, 4096), (128, True, 8192)):
        stride = R.stride_of(safe)
        start = (rng.getrandbits(bits) | (3 << (bits - 2))) // stride * stride + (3 if safe else 1)
        offs, survivors = R.search(start, window, safe, R.PRIME_BASES, 3)
        want = [i for i in range(window) if keys._is_prime(start + stride * i) and (not safe or keys._is_prime((start + stride * i - 1) // 2))][:3]
        assert offs == want and survivors == sum(R.sieve_mask(start, window, safe)), (bits, safe)


class StubEngine:
    """an engine whose prime_search and is_prime are the models; records every call"""

    def __init__(self, empty_windows=0):
        self.calls = []
        self.empty_windows = empty_windows

    def prime_search(self, limbs, start, window, safe, bases, want=1):
        start = sum(int(w) << (64 * i) for i, w in enumerate(start))
        self.calls.append(dict(limbs=limbs, start=start, window=window, safe=safe, bases=list(bases), want=want))
        if len(self.calls) <= self.empty_windows:
            return [], 0
        offs, survivors = R.search(start, window, safe, bases, want)
        return offs, survivors

    def is_prime(self, limbs, cands, bases):
        self.calls.append(dict(limbs=limbs, bases=list(bases)))
        res = [R.mr_first_witness(sum(int(w) << (64 * i) for i, w in enumerate(c)), bases) for c in cands]
        return [f for f, _ in res], [w for _, w in res]


def _rand(seed):
    rng = random.Random(seed)
    return rng.getrandbits


@pytest.mark.parametrize("bits,safe", [(64, False), (64, True), (96, False), (128, True)])
def test_generate_prime_with_a_stub_engine(bits, safe):
    eng = StubEngine(empty_windows=2)
    p = keys.generate_prime(eng, bits, safe=safe, rounds=8, rand=_rand(bits + safe))
    assert p.bit_length() == bits and p >> (bits - 2) == 3 and keys._is_prime(p)
    assert not safe or (p % 4 == 3 and keys._is_prime((p - 1) // 2))
    assert len(eng.calls) >= 3, "two empty windows, then at least one more"
    starts = [c["start"] for c in eng.calls]
    assert len(set(starts)) == len(starts), "a fresh start per window"
    stride = 4 if safe else 2
    for c in eng.calls:
        s = c["start"]
        assert s.bit_length() == bits and s >> (bits - 2) == 3 and s % stride == (3 if safe else 1)
        assert (s + stride * (c["window"] - 1)).bit_length() == bits, "the whole window keeps the bit length"
        assert c["limbs"] == (bits + 63) // 64 and c["safe"] == safe and c["want"] == 1
        assert len(c["bases"]) == 8 and all(2 <= b < 2 ** 64 and b & 2 for b in c["bases"])
    assert len({tuple(c["bases"]) for c in eng.calls}) == len(eng.calls), "fresh bases per call"
    last = eng.calls[-1]
    assert p == last["start"] + stride * R.search(last["start"], last["window"], safe, last["bases"], 1)[0][0]


@pytest.mark.parametrize("bits,safe", [(128, False), (129, False), (128, True)])
def test_generate_key_contract(bits, safe):
    eng = StubEngine()
    p, q = keys.generate_key(eng, bits, safe=safe, rounds=8, rand=_rand(1000 + bits + safe))
    n = p * q
    assert p != q and n.bit_length() == bits and math.gcd(n, (p - 1) * (q - 1)) == 1
    assert p.bit_length() == bits // 2 and q.bit_length() == bits - bits // 2
    assert keys._is_prime(p) and keys._is_prime(q)
    if safe:
        pp, qq = (p - 1) // 2, (q - 1) // 2
        assert keys._is_prime(pp) and keys._is_prime(qq) and pp != qq
    # the dealers consume the result, and safe primes are what proves v's order
    key, shares = keys.deal_shares(p, q, 3, rand=random.Random(5).randrange)
    assert key.v_order_proved == safe and key.n == n
    assert keys.secret_from_primes(p, q)[0] == n


def test_generate_key_redraws_equal_primes():
    """a rand that repeats itself gives p == q once: generate_key draws again"""
    rng = random.Random(9)
    p0 = next(x for x in range((3 << 62) + 1, 1 << 64, 2) if keys._is_prime(x))
    first = [p0, 2, p0, 2]       # start, base, start, base: the same prime at offset 0, twice
    rand = lambda k: first.pop(0) if first else rng.getrandbits(k)
    eng = StubEngine()
    p, q = keys.generate_key(eng, 128, rounds=1, rand=rand)
    assert [c["start"] for c in eng.calls[:2]] == [p0] * 2 and len(eng.calls) >= 4
    assert p != q and (p * q).bit_length() == 128 and keys._is_prime(p) and keys._is_prime(q)


def test_is_probable_prime_with_a_stub_engine():
    eng = StubEngine()
    xs = [0, 1, 2, 3, 4, 561, 2 ** 61 - 1, 2 ** 127 - 1, (2 ** 61 - 1) ** 2, 2 ** 2048 - 1557]
    got = keys.is_probable_prime(eng, xs, rounds=16, rand=_rand(3))
    assert got == [keys._is_prime(x) for x in xs]
    assert eng.calls[0]["limbs"] == 32 and len(eng.calls[0]["bases"]) == 16 and all(b >= 2 for b in eng.calls[0]["bases"])


def test_generators_refuse_bad_arguments():
    eng = StubEngine()
    for bad in (0, 39, 2049, True, 64.0):
        with pytest.raises(ValueError):
            keys.generate_prime(eng, bad)
    for bad in (0, 65, True):
        with pytest.raises(ValueError):
            keys.generate_prime(eng, 64, rounds=bad)
    with pytest.raises(ValueError):
        keys.generate_prime(eng, 64, window=0)
    with pytest.raises(ValueError):
        keys.generate_key(eng, 64)
    with pytest.raises(ValueError):
        keys.is_probable_prime(eng, [])
    with pytest.raises(ValueError):
        keys.is_probable_prime(eng, [1 << 2048])
    with pytest.raises(ValueError):
        keys.is_probable_prime(eng, [-1])
    assert not eng.calls
    assert keys.default_window(1024, False) == 4096 and keys.default_window(1024, True) == 131072 and keys.default_window(64, True) == 1024
