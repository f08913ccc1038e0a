"""CPU: the catalogue of structured K3 operands (tests/k3_operands.py) is well formed, its model of the device's mul_mod is
consistent with Python's divmod, the catalogue reaches every (corrections, top) state random operands reach and every branch of the
normalisation shift, and the structured keys are Paillier keys.  DESIGN.md section 15.13 holds the table this file pins."""
import collections
import math
import random

import pytest

from paillier_halo2_amd import keys
from tests import decrypt_ref as DR
from tests import k3_operands as K


def _entries():
    """(limbs of the modulus, top bits, class, modulus, n or 0): the moduli taken directly, then n^2 of every n shape"""
    for limbs, tb in K.SHAPES_M:
        for cls, m in K.moduli(K.bits_of(limbs, tb)).items():
            yield limbs, tb, cls, m, 0
    for ln, tb in K.SHAPES_N:
        for cls, n in K.moduli(K.bits_of(ln, tb)).items():
            yield 2 * ln, tb, cls, n * n, n


ENTRIES = list(_entries())
CLASSES = ("all_ones", "pow2_plus1", "pow2", "minus_2_64_plus1", "alt64", "alt32_hi", "alt32_lo", "random")

# the (corrections, top) states the catalogue reaches, per modulus class (DESIGN.md section 15.13 prints this table)
STATES = {
    "all_ones": {(0, 0), (1, 0), (1, 1), (2, 1)},
    "pow2_plus1": {(0, 0), (1, 0), (1, 1), (2, 1), (3, 1)},
    "pow2": {(0, 0), (1, 0), (2, 1)},
    "minus_2_64_plus1": {(0, 0), (1, 0), (1, 1), (2, 1)},
    "alt64": {(0, 0), (1, 0), (1, 1), (2, 1), (3, 1)},
    "alt32_hi": {(0, 0), (1, 0), (1, 1), (2, 1), (2, 2)},
    "alt32_lo": {(0, 0), (1, 0), (1, 1), (2, 1), (3, 1)},
    "random": {(0, 0), (1, 0), (1, 1), (2, 1)},
}


def test_catalogue_is_well_formed():
    assert K.L_ALL == (2, 16, 18, 32, 48, 62, 64, 66, 96, 98, 128) and len(K.SHAPES_M) == len(K.SHAPES_N) == 66
    seen = collections.Counter()
    for limbs, tb in K.SHAPES_M + K.SHAPES_N:
        b = K.bits_of(limbs, tb)
        ms = K.moduli(b)
        assert len(set(ms.values())) == len(ms) and set(ms) <= set(CLASSES), (limbs, tb)
        for cls, m in ms.items():
            assert m.bit_length() == b and K.words(b) == limbs, (limbs, tb, cls)
            assert (m & 1) == (0 if cls == "pow2" and b > 1 else 1), (limbs, tb, cls)
            seen[cls] += 1
        if b > 128:
            assert set(ms) == set(CLASSES), (limbs, tb)
    assert set(seen) == set(CLASSES)
    for limbs, tb, cls, m, n in ENTRIES:
        ops = K.operands(m, limbs, n)
        assert len(set(ops.values())) == len(ops) and all(0 <= v < m for v in ops.values()), (limbs, tb, cls)
        ps = K.pairs(m, limbs, n)
        assert len(set(ps)) == len(ps) and {a for a, _ in ps} == set(ops) == {b for _, b in ps}, (limbs, tb, cls)
        vals = {(ops[a], ops[b]) for a, b in ps}
        r = math.isqrt(m)
        if m.bit_length() > 64:
            assert {0, 1, 2, m - 1, m - 2, m // 2, r, r + 1, K.alt64(m.bit_length() - 1), K.alt32_hi(m.bit_length() - 1)} <= set(ops.values())
            assert {1 << (64 * j) for j in range(K.slice_limbs(limbs), limbs, K.slice_limbs(limbs)) if 64 * j < m.bit_length() - 1} <= set(ops.values())
            assert {(m - 1, m - 1), (m - 1, 1), (r + 1, r + 1)} <= vals, (limbs, tb, cls)
        if n > 3:
            assert limbs > 18 or pow(n + 1, n - 1, m) == 1 + (n - 1) * n       # (the binomial theorem; checked where it is cheap)
            for a, b, q in ((n, n, 1), (n, 3 * n, 3), (3 * n, 3 * n, 9), ((n - 1) * n, (n - 1) * n, (n - 1) ** 2)):
                assert (a, b) in vals and divmod(a * b, m) == (q, 0), (limbs, tb, cls, q)


def test_model_is_consistent_and_the_catalogue_covers_what_random_operands_reach():
    """mul_mod_model asserts qhat + corrections == a b // m itself; here it runs over the whole catalogue and 2000 seeded random pairs
    per modulus class, and the catalogue's (corrections, top) states per class are exactly STATES, which contain the random ones"""
    cat = collections.defaultdict(set)
    by_cls = collections.defaultdict(list)
    for limbs, tb, cls, m, n in ENTRIES:
        by_cls[cls].append((limbs, m))
        ops = K.operands(m, limbs, n)
        for a, b in K.pairs(m, limbs, n):
            r = K.mul_mod_model(ops[a], ops[b], m, limbs)
            assert not r.lost and (r.q, r.r) == divmod(ops[a] * ops[b], m), (limbs, tb, cls, a, b)
            assert r.clamp == (cls == "pow2" or m == 1), (limbs, tb, cls)
            cat[cls].add((r.corrections, r.top))
    for k, cls in enumerate(CLASSES):
        rng = random.Random(0x6b00 + k)
        rnd = set()
        for i in range(2000):
            limbs, m = by_cls[cls][i % len(by_cls[cls])]
            a, b = rng.randrange(m), rng.randrange(m)
            r = K.mul_mod_model(a, b, m, limbs)
            assert not r.lost and (r.q, r.r) == divmod(a * b, m)
            rnd.add((r.corrections, r.top))
        assert cat[cls] == STATES[cls], cls
        assert rnd <= cat[cls], (cls, rnd - cat[cls])
        assert max(c for c, _ in cat[cls] | rnd) <= 3 and all(t <= c for c, t in cat[cls] | rnd), cls


def test_model_flags_exactly_the_quotients_that_do_not_fit():
    """over the unreduced pairs: `lost` (the capacity) implies a quotient beyond `limbs` limbs, and where nothing is lost the model's
    quotient is divmod's, which the device then holds to `limbs` limbs (ld_exceeds)"""
    fits = collections.Counter()
    for limbs, tb, cls, m, n in ENTRIES:
        if n:
            continue
        un = K.unreduced(m, limbs)
        for a, b in K.UNREDUCED_PAIRS:
            r = K.mul_mod_model(un[a], un[b], m, limbs)
            big = un[a] * un[b] // m >> (64 * limbs) != 0
            assert (not r.lost) or big, (limbs, tb, cls, a, b)
            assert r.lost or (r.q, r.r) == divmod(un[a] * un[b], m)
            fits[big] += 1
    assert fits[True] > 1000 and fits[False] > 1000


def test_catalogue_reaches_every_branch_of_the_normalisation_shift():
    paths = collections.defaultdict(set)
    for limbs, tb, cls, m, n in ENTRIES:
        E, N, s, _, _ = K.barrett(m, limbs)
        paths[K.shift_path(E, s >> 6, s & 63)].add((limbs, tb, bool(n)))
    want = {"dpp bs=0", "dpp bs=1", "dpp bs>=62", "dpp", "lds ls=1 bs=0", "lds ls=1 bs!=0", "lds ls>=2 bs=0", "lds ls>=2 bs!=0",
            "lds E=2 ls=0 bs=0", "lds E=2 ls=0 bs!=0", "lds E=2 ls>=1 bs=0", "lds E=2 ls>=1 bs!=0"}
    assert set(paths) == want
    # ls = 1 at E = 1 needs a 63-limb modulus: only n^2 of a 32-limb n with a short top limb gets there
    assert all(sq for p in ("lds ls=1 bs=0", "lds ls=1 bs!=0") for _, _, sq in paths[p])
    # the production case -- n^2 of a full-size key -- is on the DPP path, with and without a bit shift
    assert (64, 64, True) in paths["dpp bs=0"] | paths["dpp bs=1"] and (64, 63, True) in paths["dpp"] | paths["dpp bs=1"] | paths["dpp bs>=62"]
    for which, bs in (("mixed", 1), ("high", 0)):
        p, q = K.structured_key_primes(which)
        E, N, s, _, _ = K.barrett((p * q) ** 2, 64)
        assert (E, s) == (1, bs), which


def _cts(k, p, q):
    """1, n + 1, 1 + (n - 1) n, n^2 - 1, encryptions of 0, 1 and n - 1 (under r in {1, n - 1, 2^k}; above 1200 bits under one r each, for the
    time), two non-units"""
    n, g = k[0], k[1]
    rs = (1, n - 1, 1 << (n.bit_length() // 2))
    pairs = [(m, r) for m in (0, 1, n - 1) for r in rs] if n.bit_length() <= 1200 else list(zip((0, 1, n - 1), rs))
    return [1, n + 1, 1 + (n - 1) * n, n * n - 1], pairs, [p, p * (q - 2)]


@pytest.mark.parametrize("i", range(len(K.MERSENNE)))
def test_mersenne_keys_are_paillier_keys(i):
    p, q = K.mersenne_primes(i)
    assert keys._is_prime(p) and keys._is_prime(q)
    n, g, lam, d = keys.secret_from_primes(p, q)
    a, b = K.MERSENNE[i]
    assert n == (1 << (a + b)) - (1 << a) - (1 << b) + 1 and n.bit_length() == K.MERSENNE_BITS[i]
    assert [K.words(x) for x in K.MERSENNE_BITS] == [3, 4, 4, 11, 18, 30, 55]
    k = K.full_key(p, q)
    assert k[:4] == (n, g, lam, d)
    _round_trip(k, p, q)
    if i < 4:       # a general g, found as tests/decrypt_ref.key finds it
        gg = K.general_g(n, lam, i)
        assert keys.secret_from_primes(p, q, gg)[1] == gg
        _round_trip(K.full_key(p, q, gg), p, q)


def _round_trip(k, p, q):
    from tests import shamir_ref as SR

    n, g = k[0], k[1]
    fixed, pairs, bad = _cts(k, p, q)
    assert [DR.decrypt_ref(k, SR.encrypt(n, g, m, r, pq=(p, q))) for m, r in pairs] == [(m, r, 0) for m, r in pairs]
    assert [DR.decrypt_ref(k, c) for c in bad] == [(0, 0, 1)] * 2 and DR.decrypt_ref(k, 1) == (0, 1, 0)
    for c in fixed[1:]:
        m, r, flag = DR.decrypt_ref(k, c)
        assert flag == 0 and SR.encrypt(n, g, m, r, pq=(p, q)) == c


@pytest.mark.parametrize("which", K.STRUCTURED_KEYS)
def test_structured_prime_keys_are_paillier_keys(which):
    d = K.structured_primes()
    for kk, v in d.items():
        kk = int(kk)
        assert keys._is_prime((1 << kk) - v["c1"]) and keys._is_prime((1 << kk) - v["c2"]) and keys._is_prime((1 << (kk - 1)) + v["c_low"])
        assert 0 < v["c1"] < v["c2"]
    v = d["256"]            # minimality, checked where it is cheap
    assert not any(keys._is_prime((1 << 256) - c) for c in range(1, v["c2"]) if c != v["c1"])
    assert not any(keys._is_prime((1 << 255) + c) for c in range(1, v["c_low"]))
    p, q = K.structured_key_primes(which)
    n, g, lam, dd = keys.secret_from_primes(p, q)
    assert n.bit_length() == 2048 and (n * n).bit_length() == (4095 if which == "mixed" else 4096)
    assert math.gcd(n, lam) == 1
    _round_trip(K.full_key(p, q), p, q)
