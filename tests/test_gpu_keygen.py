"""GPU: prime generation on the device -- pz_bigint_is_prime's flags and witness indices against
tests/prime_ref.py entry for entry over the catalogue, pz_prime_sieve's mask bit for bit, pz_prime_search's offsets, found and survivor
count for starts chosen beforehand with the model, every refusal, and keys.generate_key end to end into the dealers, the combiner and
the secret-key handle.  Every comparison is exact."""
import functools
import math
import random

import numpy as np
import pytest

from tests import prime_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _rows(cs, limbs):
    return np.array([R.words(c, limbs) for c in cs], dtype=np.uint64).reshape(len(cs), limbs)


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


def _check(eng, limbs, cs, bases):
    flags, wit = eng.is_prime(limbs, _rows(cs, limbs), np.array(bases, dtype=np.uint64))
    want = [R.mr_first_witness(c, bases) for c in cs]
    got = list(zip(flags.tolist(), wit.tolist()))
    bad = [(j, hex(cs[j]), got[j], want[j]) for j in range(len(cs)) if got[j] != want[j]]
    assert not bad, bad[:8]


# ------------------------------------------------------------------------------------------------------------------ 1. Miller-Rabin
@pytest.mark.parametrize("limbs", [1, 2, 15, 16, 17, 32])
def test_catalogue_flags_and_witness_indices(eng, limbs):
    """every catalogue value that fits, small values with leading zero limbs included; then the bases that reduce to 0, 1 and c - 1"""
    cs = [c for _, c, _ in R.CATALOGUE if R.fits(c, limbs)]
    assert len(cs) >= 20 and (limbs < 32 or len(cs) == len(R.CATALOGUE))
    _check(eng, limbs, cs, R.PRIME_BASES)
    for c, bases, wit in R.REDUCING:
        if R.fits(c, limbs):
            assert R.mr_first_witness(c, bases)[1] == wit
            _check(eng, limbs, [c, c + 2, c], bases)


@pytest.mark.parametrize("limbs", [2, 17])
@pytest.mark.parametrize("count", [1, 3, 5, 257])
def test_partial_wavefronts_and_blocks(eng, limbs, count):
    """four candidates per wavefront, sixteen per workgroup: counts that leave groups of the last wavefront and workgroup idle"""
    rng = random.Random(0x6b00 + 64 * limbs + count)
    pool = [c for _, c, _ in R.CATALOGUE if R.fits(c, limbs)]
    cs = [pool[(7 * j + count) % len(pool)] if j % 3 else rng.getrandbits(64 * limbs) | 1 for j in range(count)]
    _check(eng, limbs, cs, R.PRIME_BASES[:4])


@pytest.mark.parametrize("rounds", [1, 64])
def test_round_counts(eng, rounds):
    rng = random.Random(0x6b10 + rounds)
    bases = [rng.getrandbits(64) | 2 for _ in range(rounds)]
    cs = [c for _, c, _ in R.CATALOGUE if R.fits(c, 16)][::3] + [561, 2 ** 64 + 1]
    _check(eng, 16, cs, bases)
    # a composite that fails only in the last round: 2^64 + 1 passes base 2 and its powers
    liars = [2 ** (k % 63 + 1) for k in range(rounds - 1)] + [3]
    assert R.mr_first_witness(2 ** 64 + 1, liars) == (0, rounds - 1)
    _check(eng, 2, [2 ** 64 + 1, 2 ** 64 + 13], liars)


def test_device_form(eng):
    import torch

    limbs = 17
    cs = [c for _, c, _ in R.CATALOGUE if R.fits(c, limbs)]
    count = len(cs)
    d_c = torch.from_numpy(_rows(cs, limbs).astype(np.int64)).cuda()
    d_fl = torch.full((count,), 0xEE, dtype=torch.uint8, device="cuda")
    d_w = torch.full((count,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()
    eng.is_prime_dev(limbs, count, d_c.data_ptr(), np.array(R.PRIME_BASES, dtype=np.uint64), d_fl.data_ptr(), d_w.data_ptr())
    eng.sync()
    want = [R.mr_first_witness(c, R.PRIME_BASES) for c in cs]
    assert list(zip(d_fl.cpu().tolist(), d_w.cpu().numpy().view(np.uint32).tolist())) == want


def test_is_prime_refusals_come_before_any_launch(eng):
    import torch
    from paillier_halo2_amd import _lib

    L, ctx, p = eng.L, eng.ctx, lambda a: None if a is None else a.ctypes.data
    c = _rows([2 ** 61 - 1, 561], 33)
    b, small = np.array([2, 3], dtype=np.uint64), np.array([2, 1], dtype=np.uint64)
    f, w = np.full(2, 0xEE, dtype=np.uint8), np.full(2, 0xABCD, dtype=np.uint32)
    d_c = torch.from_numpy(c.astype(np.int64)).cuda()
    d_f = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    d_w = torch.full((2,), 0xABCD, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()
    for fn, cc, ff, ww in ((L.pz_bigint_is_prime, p(c), p(f), p(w)), (L.pz_bigint_is_prime_dev, d_c.data_ptr(), d_f.data_ptr(), d_w.data_ptr())):
        def call(limbs=2, count=2, cands=cc, rounds=2, bases=b, flags=ff, wit=ww):
            return fn(ctx, limbs, count, cands, rounds, p(bases), flags, wit)

        for kw in (dict(cands=None), dict(bases=None), dict(flags=None), dict(wit=None), dict(limbs=0), dict(count=0), dict(count=65537),
                   dict(rounds=0), dict(rounds=65), dict(bases=small), dict(limbs=33, bases=small), dict(limbs=33, count=0)):
            assert call(**kw) == _lib.PZ_ERR_INVALID, kw
        assert fn(None, 2, 2, cc, 2, p(b), ff, ww) == _lib.PZ_ERR_INVALID
        assert call(limbs=33) == _lib.PZ_ERR_UNSUPPORTED
    eng.sync()
    assert f.tolist() == [0xEE] * 2 and w.tolist() == [0xABCD] * 2, "the outputs are untouched"
    assert d_f.cpu().tolist() == [0xEE] * 2 and d_w.cpu().tolist() == [0xABCD] * 2, "the device outputs are untouched"


# ------------------------------------------------------------------------------------------------------------------ 2. the sieve
def _start(bits, safe, seed):
    x = random.Random(seed).getrandbits(bits) | (3 << (bits - 2))
    return x - x % 4 + 3 if safe else x | 1


@pytest.mark.parametrize("safe", [False, True])
@pytest.mark.parametrize("bits", [64, 128, 1024])
def test_sieve_mask_equals_the_model(eng, bits, safe):
    limbs = bits // 64
    start = _start(bits, safe, 0x6c00 + bits)
    for window in (1, 63, 64, 65, 4096):
        mask = eng.prime_sieve(limbs, R.words(start, limbs), window, safe)
        assert mask.tobytes() == R.sieve_mask(start, window, safe), (bits, safe, window)
    assert 0 < sum(R.sieve_mask(start, 4096, safe)) < 4096 // 4


@pytest.mark.parametrize("safe", [False, True])
def test_sieve_at_the_top_of_the_word_range_and_refusals(eng, safe):
    from paillier_halo2_amd import _lib

    stride, window = R.stride_of(safe), 4097
    for limbs in (1, 3):
        top = (1 << (64 * limbs)) - 1                       # odd, and 3 mod 4
        start = top - stride * (window - 1)
        mask = eng.prime_sieve(limbs, R.words(start, limbs), window, safe)
        assert mask.tobytes() == R.sieve_mask(start, window, safe)
        assert _status(lambda: eng.prime_sieve(limbs, R.words(start + stride, limbs), window, safe)) == _lib.PZ_ERR_RANGE
    L, ctx, p = eng.L, eng.ctx, lambda a: None if a is None else a.ctypes.data
    good = np.array(R.words(_start(128, safe, 5), 33), dtype=np.uint64)
    low = np.array(R.words((1 << 32) - 1, 33), dtype=np.uint64)        # below 2^32 (odd, 3 mod 4)
    even = good.copy()
    even[0] -= 1                                                       # even; 2 mod 4
    one_mod_4 = good.copy()
    one_mod_4[0] -= 2
    out = np.full(64, 0xEE, dtype=np.uint8)

    def call(limbs=2, start=good, window=64, safe_=int(safe), mask=out):
        return L.pz_prime_sieve(ctx, limbs, p(start), window, safe_, p(mask))

    for kw in (dict(start=None), dict(mask=None), dict(limbs=0), dict(window=0), dict(window=(1 << 20) + 1), dict(safe_=2), dict(start=low),
               dict(start=even), dict(limbs=0, start=low)):
        assert call(**kw) == _lib.PZ_ERR_INVALID, kw
    if safe:
        assert call(start=one_mod_4) == _lib.PZ_ERR_INVALID
    assert call(limbs=33) == _lib.PZ_ERR_UNSUPPORTED and call(limbs=33, start=low) == _lib.PZ_ERR_UNSUPPORTED
    assert out.tolist() == [0xEE] * 64, "the mask is untouched by a refusal"


# ------------------------------------------------------------------------------------------------------------------ 3. the search
SEARCH_BASES = tuple(random.Random(0x6d00).getrandbits(64) | 2 for _ in range(8))


@functools.lru_cache(maxsize=None)
def _gap_start():
    """the odd number after a 64-bit prime that is followed by at least nine composites at stride 2"""
    from paillier_halo2_amd import keys

    x = (3 << 62) + 1
    while True:
        if keys._is_prime(x) and not any(keys._is_prime(x + 2 * i) for i in range(1, 10)):
            return x + 2
        x += 2


SEARCHES = {
    # name: (bits, safe, window, how many the model must find, the seed of the start)
    "64 plain": (64, False, 4096, 3, 0x6d10),
    "64 safe": (64, True, 4096, 3, 0x6d13),
    "256 safe": (256, True, 1 << 16, 1, 0x6d10),
    "1024 plain": (1024, False, 4096, 1, 0x6d10),
}


@functools.lru_cache(maxsize=None)
def _search_case(name):
    """(start, window, safe, the model's (offsets, survivors) for want = 3): the start is fixed by a seed and must satisfy the condition
    the test is about -- the model finds at least `need` in the window"""
    bits, safe, window, need, seed = SEARCHES[name]
    start = _start(bits, safe, seed)
    offs, survivors = R.search(start, window, safe, SEARCH_BASES, 3)
    assert len(offs) >= need, "a condition of the test: choose another seed"
    return start, window, safe, offs, survivors


@pytest.mark.parametrize("want", [1, 3])
@pytest.mark.parametrize("name", list(SEARCHES))
def test_search_equals_the_model(eng, name, want):
    start, window, safe, offs, survivors = _search_case(name)
    limbs = SEARCHES[name][0] // 64
    got, surv = eng.prime_search(limbs, R.words(start, limbs), window, safe, np.array(SEARCH_BASES, dtype=np.uint64), want)
    assert (got.tolist(), surv) == (offs[:want], survivors)


def test_search_inside_a_prime_gap_finds_nothing(eng):
    start = _gap_start()
    assert R.search(start, 8, False, SEARCH_BASES, 3) == ([], sum(R.sieve_mask(start, 8, False)))
    got, surv = eng.prime_search(1, R.words(start, 1), 8, False, np.array(SEARCH_BASES, dtype=np.uint64), 3)
    assert (got.tolist(), surv) == ([], sum(R.sieve_mask(start, 8, False)))


def test_search_with_one_round_and_refusals(eng):
    from paillier_halo2_amd import _lib

    start, window, safe, _, survivors = _search_case("64 safe")
    one = SEARCH_BASES[:1]
    got, surv = eng.prime_search(1, R.words(start, 1), window, safe, np.array(one, dtype=np.uint64), 64)
    assert (got.tolist(), surv) == R.search(start, window, safe, one, 64)
    L, ctx, p = eng.L, eng.ctx, lambda a: None if a is None else a.ctypes.data
    import ctypes as C

    s = np.array(R.words(start, 33), dtype=np.uint64)
    low = np.array(R.words((1 << 32) - 1, 33), dtype=np.uint64)
    even = s.copy()
    even[0] -= 1
    b, small = np.array(SEARCH_BASES, dtype=np.uint64), np.array([2, 0], dtype=np.uint64)
    offs, found = np.full(64, 0xABCD, dtype=np.uint32), C.c_uint32(77)

    def call(limbs=1, start=s, window=64, safe_=1, rounds=2, bases=b, want=3, offsets=offs, fnd=C.byref(found), surv=None):
        return L.pz_prime_search(ctx, limbs, p(start), window, safe_, rounds, p(bases), want, p(offsets), fnd, surv)

    for kw in (dict(start=None), dict(bases=None), dict(offsets=None), dict(fnd=None), dict(limbs=0), dict(window=0), dict(window=(1 << 20) + 1),
               dict(safe_=2), dict(rounds=0), dict(rounds=65), dict(bases=small), dict(want=0), dict(want=65), dict(start=low), dict(safe_=0, start=even),
               dict(limbs=33, want=0)):
        assert call(**kw) == _lib.PZ_ERR_INVALID, kw
    assert call(limbs=33) == _lib.PZ_ERR_UNSUPPORTED
    top = np.array(R.words(2 ** 64 - 1, 1), dtype=np.uint64)
    assert call(start=top, window=2) == _lib.PZ_ERR_RANGE
    assert offs.tolist() == [0xABCD] * 64 and found.value == 77, "the outputs are untouched by a refusal"


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
def test_safe_key_end_to_end_into_the_dealer_and_the_combiner(eng):
    """keys.generate_key(safe) -> deal_shares proves v's order -> three trustees open a ciphertext with the device's partial / combine"""
    from paillier_halo2_amd import keys
    from tests import partial_ref as TR

    rng = random.Random(0x6e00)
    p, q = keys.generate_key(eng, 256, safe=True, rounds=16, rand=rng.getrandbits)
    n = p * q
    assert p != q and n.bit_length() == 256 and math.gcd(n, (p - 1) * (q - 1)) == 1
    assert all(keys._is_prime(x) for x in (p, q, (p - 1) // 2, (q - 1) // 2)) and p % 4 == q % 4 == 3
    assert keys.is_probable_prime(eng, [p, q, (p - 1) // 2, n, p + 2], rand=rng.getrandbits)[:4] == [True, True, True, False]
    key, shares = keys.deal_shares(p, q, 3, rand=rng.randrange)
    assert key.v_order_proved is True
    Ln, m = 4, rng.randrange(n)
    c = pow(key.g, m, n * n) * pow(rng.randrange(1, n), n, n * n) % (n * n)
    lim = lambda x, k: np.array(R.words(x, k), dtype=np.uint64)
    parts = []
    for s, h in zip(shares, key.hs):
        hh, u, _ = eng.paillier_partial(Ln, lim(n, Ln), lim(key.v, 2 * Ln), lim(s, 2 * Ln), lim(c, 2 * Ln).reshape(1, -1), 2 * 256, want_steps=False)
        assert sum(int(v) << (64 * i) for i, v in enumerate(hh)) == h
        assert sum(int(v) << (64 * i) for i, v in enumerate(u[0])) == TR.partial(c, s, n)
        parts.append(u)
    got, flags = eng.paillier_combine(Ln, lim(n, Ln), lim(key.mu2, Ln), np.stack(parts))
    assert (sum(int(v) << (64 * i) for i, v in enumerate(got[0])), flags.tolist()) == (m, [0])


def test_2048_bit_key_satisfies_the_contract_and_the_key_handle_accepts_it(eng):
    from paillier_halo2_amd import keys

    rng = random.Random(0x6e10)
    p, q = keys.generate_key(eng, 2048, rand=rng.getrandbits)
    n = p * q
    assert p != q and n.bit_length() == 2048 and p.bit_length() == q.bit_length() == 1024 and math.gcd(n, (p - 1) * (q - 1)) == 1
    assert keys._is_prime(p) and keys._is_prime(q)
    sk = eng.paillier_sk(32, *keys.secret_from_primes(p, q))
    try:
        m = rng.randrange(n)
        c = (1 + m * n) * pow(rng.randrange(1, n), n, n * n) % (n * n)
        got, _, flags = eng.paillier_decrypt(sk, np.array(R.words(c, 64), dtype=np.uint64).reshape(1, -1), want_r=False)
        assert (sum(int(v) << (64 * i) for i, v in enumerate(got[0])), flags.tolist()) == (m, [0])
    finally:
        sk.free()
