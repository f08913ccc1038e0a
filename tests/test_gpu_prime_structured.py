"""GPU: the prime generation held to Python integers on structured operands.  The group arithmetic of
csrc/prime_mont.cuh one function at a time through the probe library (probe.prime_ops) over the catalogue of tests/prime_operands.py:
mont_mul over every shape x class x pair with every triple in every group position of a wavefront, prime_setup, grp_sub, grp_double_mod
and the triples found by search; then pz_bigint_is_prime on structured primes at every limb count 1 .. 32, the sieve's mask bit for bit
past its first segments, and searches that cross a batch.  Every comparison is exact."""
import functools
import random

import numpy as np
import pytest

from tests import prime_operands as PO
from tests import prime_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _rows(vals, limbs):
    buf = b"".join(v.to_bytes(8 * limbs, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(len(vals), limbs).astype(np.uint64)


def _ints(arr):
    return [int.from_bytes(np.ascontiguousarray(row, dtype="<u8").tobytes(), "little") for row in arr]


def _op(op, limbs, a=None, b=None, c=None):
    from paillier_halo2_amd import probe

    out, flag = probe.prime_ops(0, op, limbs, *(None if x is None else _rows(x, limbs) for x in (a, b, c)))
    return out, flag.tolist()


def _first_diff(got, want):
    bad = [(j, hex(g), hex(w)) for j, (g, w) in enumerate(zip(got, want)) if g != w]
    return (len(bad), bad[:3])


@functools.lru_cache(maxsize=None)
def _rinv(c, limbs):
    return pow(1 << (64 * limbs), -1, c)


def _uneven(items):
    """a count that is no multiple of 4 (so none of 16 either): the last wavefront and block keep idle groups"""
    items = list(items)
    while len(items) % 4 == 0:
        items.append(items[len(items) // 2])
    return items


# ------------------------------------------------------------------------------------------------------------------ 1. the probe ops
@pytest.mark.parametrize("limbs", PO.LIMBS_ALL)
def test_mont_mul_over_every_shape_class_and_pair(limbs):
    tr = _uneven((a, b, c) for _, a, b, c in PO.triples(limbs))
    want = [a * b * _rinv(c, limbs) % c for a, b, c in tr]
    assert len(tr) % 4 != 0 and len(tr) > 500
    for rot in range(4):            # every triple in every group of a wavefront
        t, w = tr[rot:] + tr[:rot], want[rot:] + want[:rot]
        out, _ = _op("mont_mul", limbs, *zip(*t))
        assert _first_diff(_ints(out), w) == (0, []), (limbs, rot)


def test_setup_for_every_modulus():
    for limbs in PO.LIMBS_ALL:
        cs = _uneven(c for tb in PO.TOP_BITS for c in PO.moduli(limbs, tb).values())
        out, ninv = _op("setup", limbs, c=cs)
        Rr = 1 << (64 * limbs)
        assert _first_diff(_ints(out[:, :limbs]), [Rr % c for c in cs]) == (0, []), limbs
        assert _first_diff(_ints(out[:, limbs:]), [Rr * Rr % c for c in cs]) == (0, []), limbs
        assert ninv == [-pow(c, -1, 1 << 64) % (1 << 64) for c in cs], limbs


def test_sub_on_moduli_and_on_operands_equal_in_all_but_one_lane():
    for limbs in PO.LIMBS_ALL:
        E = PO.capacity(limbs)
        W, Rr = 1 << (64 * 16 * E), 1 << (64 * limbs)
        ab = []
        for tb in PO.TOP_BITS:
            for c in PO.moduli(limbs, tb).values():
                ab.append((c, Rr % c))
                ab += [(x, c) for x in PO.operands_a(c, limbs).values()]
        x = PO.pattern("hi32_1", limbs)
        for k in range(0, limbs, E):            # equal in all but lane k / E: the borrow, or none, crosses every lane above
            ab += [(x, x + (1 << (64 * k))), (x + (1 << (64 * k)), x), (x, x ^ (1 << (64 * k + 63))), (x ^ (1 << (64 * (k + E) - 1)), x)]
        ab = _uneven((a, b) for a, b in ab if a < Rr and b < Rr)
        for rot in (0, 1, 2, 3):
            t = ab[rot:] + ab[:rot]
            out, borrow = _op("sub", limbs, a=[a for a, _ in t], b=[b for _, b in t])
            assert out.shape[1] == 16 * E
            assert _first_diff(_ints(out), [(a - b) % W for a, b in t]) == (0, []), (limbs, rot)
            assert borrow == [int(a < b) for a, b in t], (limbs, rot)


def test_double_mod_on_one_hot_operands_and_c_minus_1():
    for limbs in PO.LIMBS_ALL:
        E = PO.capacity(limbs)
        xc = []
        for tb in PO.TOP_BITS:
            for c in PO.moduli(limbs, tb).values():
                xs = [c - 1, c // 2, (c + 1) // 2] + [1 << (64 * j - 1) for j in range(E, limbs + 1, E)] + [1 << (64 * j) for j in range(0, limbs, E)]
                xc += [(x, c) for x in xs if x < c]
        xc = _uneven(xc)
        out, _ = _op("double_mod", limbs, a=[x for x, _ in xc], c=[c for _, c in xc])
        assert _first_diff(_ints(out), [2 * x % c for x, c in xc]) == (0, []), limbs


@pytest.mark.parametrize("case", range(len(PO.SEARCHED)))
def test_searched_triples_in_every_group_position(case):
    limbs, cls, seed, target, state = PO.SEARCHED[case]
    a, b, c = PO.searched_triple(limbs, cls, seed, target)
    s = PO.mont_mul_model(a, b, c, limbs)
    assert PO.searched_state(s) == state
    fill = [(x, y, z) for _, x, y, z in PO.triples(limbs)[:3]]
    tr = [(a, b, c)] * 4 + fill + [(a, b, c)] * 4 + fill[:2]            # 16 groups of one block, then a second block
    tr = tr + tr[:5]
    out, _ = _op("mont_mul", limbs, *zip(*tr))
    assert _first_diff(_ints(out), [x * y * _rinv(z, limbs) % z for x, y, z in tr]) == (0, [])
    assert _ints(out)[0] == s.r


def test_probe_refusals_come_before_any_launch():
    from paillier_halo2_amd import probe

    one = lambda v, limbs=2: _rows([v], limbs)
    good = dict(a=one(5), b=one(7), c=one(11))
    probe.prime_ops(0, "mont_mul", 2, **good)
    for kw in (dict(good, c=one(10)), dict(good, c=one(1)), dict(good, a=one(11)), dict(good, a=one(12)), dict(good, c=one(1 << 64 | 2))):
        with pytest.raises(RuntimeError):
            probe.prime_ops(0, "mont_mul", 2, **kw)
    with pytest.raises(RuntimeError):
        probe.prime_ops(0, "double_mod", 2, a=one(11), c=one(11))
    with pytest.raises(RuntimeError):
        probe.prime_ops(0, "setup", 2, c=one(2))
    l = probe.lib()
    buf = np.zeros(33 * 4, dtype=np.uint64)
    p = buf.ctypes.data
    assert l.pzp_prime_ops(0, 0, 0, 1, p, p, p, p, p) == -1 and l.pzp_prime_ops(0, 0, 33, 1, p, p, p, p, p) == -1
    assert l.pzp_prime_ops(0, 0, 2, 0, p, p, p, p, p) == -1 and l.pzp_prime_ops(0, 0, 2, 65537, p, p, p, p, p) == -1
    assert l.pzp_prime_ops(0, 4, 2, 1, p, p, p, p, p) == -1 and l.pzp_prime_ops(0, -1, 2, 1, p, p, p, p, p) == -1


# ------------------------------------------------------------------------------------------------------------------ 2. Miller-Rabin
def _check(eng, limbs, cs, bases, want=None):
    flags, wit = eng.is_prime(limbs, _rows(cs, limbs), np.array(bases, dtype=np.uint64))
    want = want or [R.mr_first_witness(c, bases) for c in cs]
    got = list(zip(flags.tolist(), wit.tolist()))
    bad = [(j, hex(cs[j]), got[j], want[j]) for j in range(len(cs)) if got[j] != want[j]]
    assert not bad, (limbs, bad[:4])


@functools.lru_cache(maxsize=None)
def _primes_at(limbs):
    return tuple(dict.fromkeys(PO.pattern_prime(l, n, k, s) for l, n, k, s in PO.structured_primes() if l == limbs))


@pytest.mark.parametrize("limbs", PO.LIMBS_ALL)
def test_structured_primes_at_their_own_limb_count_and_wider(eng, limbs):
    ps = list(_primes_at(limbs))
    rounds = len(PO.STRUCT_BASES)
    assert rounds == 21 and ps and all(p.bit_length() == 64 * limbs for p in ps)
    near = [p + d for p in ps for d in (-2, 2) if p + d < 1 << (64 * limbs)]
    cs = ps + near
    _check(eng, limbs, cs, PO.STRUCT_BASES, [(1, rounds)] * len(ps) + [R.mr_first_witness(c, PO.STRUCT_BASES) for c in near])
    for wider in sorted({limbs + 1, 16, 32}):
        if limbs < wider <= 32:
            _check(eng, wider, ps, PO.STRUCT_BASES[14:], [(1, rounds - 14)] * len(ps))


def test_proth_primes_with_bases_that_reach_minus_one_at_each_position(eng):
    for s, k, z in PO.proth_primes():
        c = k * 2 ** s + 1
        limbs = PO.nwords(c.bit_length())
        bases = [z ** (2 ** j) for j in range(6) if z ** (2 ** j) < 1 << 64]
        assert all(PO.first_minus_one(c, b) == s - 1 - j for j, b in enumerate(bases))
        # one round each, so that a base's own position decides the flag; then all together
        for b in bases:
            _check(eng, limbs, [c, c + 2, c], [b], [(1, 1), R.mr_first_witness(c + 2, [b]), (1, 1)])
        _check(eng, limbs, [c, c - 2, c + 2], bases + list(R.PRIME_BASES))


@pytest.mark.parametrize("limbs", [1, 2, 17])
def test_small_negatives(eng, limbs):
    cs = list(PO.SMALL_NEGATIVES)
    assert R.mr_first_witness(341, (2,)) == (0, 0)
    _check(eng, limbs, cs, (2,))
    _check(eng, limbs, cs + [c + 2 for c in cs], R.PRIME_BASES)
    # bases coprime to a Carmichael number give a^(c-1) = 1 and still fail: no -1 on the way
    _check(eng, limbs, cs, (2, 4, 16, 256, 65536, 2 ** 32, 2 ** 63))


@pytest.mark.parametrize("limbs", [24, 31])
def test_device_form_at_24_and_31_limbs(eng, limbs):
    import torch

    ps = list(_primes_at(limbs))
    cs = ps + [p - 2 for p in ps] + [c for _, c, _ in R.CATALOGUE if R.fits(c, limbs)][::5]
    count = len(cs)
    d_c = torch.from_numpy(_rows(cs, limbs).astype(np.int64)).cuda()
    d_fl = torch.full((count,), 0xEE, dtype=torch.uint8, device="cuda")
    d_w = torch.full((count,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()
    eng.is_prime_dev(limbs, count, d_c.data_ptr(), np.array(R.PRIME_BASES, dtype=np.uint64), d_fl.data_ptr(), d_w.data_ptr())
    eng.sync()
    want = [R.mr_first_witness(c, R.PRIME_BASES) for c in cs]
    assert want[:len(ps)] == [(1, R.ALL_PASS)] * len(ps)
    assert list(zip(d_fl.cpu().tolist(), d_w.cpu().numpy().view(np.uint32).tolist())) == want


# ------------------------------------------------------------------------------------------------------------------ 3. the sieve
WINDOWS = (4095, 8193, 12289, 65537, 1 << 20)


def _start(bits, safe, seed):
    x = random.Random(seed).getrandbits(bits) | (3 << (bits - 2))
    return x - x % 4 + 3 if safe else x | 1


def _with_residues(start, want):
    """start + 4 t (so its residue modulo 4 stays) with the residue want[p] modulo every prime p of `want`"""
    t, m = 0, 1
    for p, r in want.items():
        need = (r - start) * pow(4, -1, p) % p
        t += m * ((need - t) * pow(m, -1, p) % p)
        m *= p
    out = start + 4 * t
    assert all(out % p == r % p for p, r in want.items()) and out % 4 == start % 4
    return out


@functools.lru_cache(maxsize=None)
def _mask(start, safe):
    """the model's mask over the largest window, computed once: a smaller window's mask is its prefix"""
    return R.sieve_mask(start, WINDOWS[-1], safe)


@pytest.mark.parametrize("safe", [False, True])
@pytest.mark.parametrize("bits", [64, 1024])
def test_sieve_mask_past_the_first_segments(eng, bits, safe):
    limbs = bits // 64
    start = _start(bits, safe, 0x7d00 + bits) - (1 << (bits - 2))          # room for start + stride 2^20 inside the limbs
    want = _mask(start, safe)
    for window in WINDOWS:
        mask = eng.prime_sieve(limbs, R.words(start, limbs), window, safe)
        assert mask.tobytes() == want[:window], (bits, safe, window)


@pytest.mark.parametrize("safe", [False, True])
def test_sieve_starts_at_chosen_residues(eng, safe):
    stride, window = R.stride_of(safe), 12289
    base = _start(128, safe, 0x7d10)
    starts = [_with_residues(base, {p: r}) for p in (3, 4093, 4099, 65521) for r in (0, 1, p - 1)]
    # a multiple exactly on offsets 4095 and 4096 (the last of a segment, the first of the next) and on window - 1
    edge = _with_residues(base, {4093: -stride * 4095, 4099: -stride * 4096, 65521: -stride * (window - 1)})
    for start in starts + [edge]:
        want = R.sieve_mask(start, window, safe)
        mask = eng.prime_sieve(2, R.words(start, 2), window, safe)
        assert mask.tobytes() == want, hex(start)
    want = R.sieve_mask(edge, window, safe)
    assert want[4095] == want[4096] == want[window - 1] == 0


# ------------------------------------------------------------------------------------------------------------------ 4. the search
SEARCH_BASES = tuple(random.Random(0x6d00).getrandbits(64) | 2 for _ in range(8))
CROSSING = {
    # name: (bits, safe, window, want, seed, the batch the last prime's survivor rank must exceed)
    "plain past 1024 survivors": (512, False, 1 << 15, 64, 1, 1024),
    "safe past 4096 survivors": (384, True, 1 << 20, 32, 1, 4096),
}


@pytest.mark.parametrize("name", list(CROSSING))
def test_search_crosses_a_batch(eng, name):
    bits, safe, window, want, seed, batch = CROSSING[name]
    limbs = bits // 64
    start = _start(bits, safe, seed)
    offs, survivors = R.search(start, window, safe, SEARCH_BASES, want)
    mask = R.sieve_mask(start, window, safe)
    assert len(offs) == want and sum(mask[:offs[-1] + 1]) > batch, "a condition of the test: choose another seed"
    got, surv = eng.prime_search(limbs, R.words(start, limbs), window, safe, np.array(SEARCH_BASES, dtype=np.uint64), want)
    assert (got.tolist(), surv) == (offs, survivors)


@pytest.mark.parametrize("safe", [False, True])
@pytest.mark.parametrize("limbs", [3, 16, 32])
def test_search_from_a_start_whose_carries_ripple_to_the_top_limb(eng, limbs, safe):
    """every limb below the top one all ones (odd, and 3 mod 4): any offset but 0 carries into the top limb, in the candidates and, with
    safe, in their halves"""
    top = random.Random(0x7e00 + limbs).getrandbits(62) | (1 << 61)
    start = (top << (64 * (limbs - 1))) | ((1 << (64 * (limbs - 1))) - 1)
    window = 1 << 14 if limbs == 3 else 2048
    offs, survivors = R.search(start, window, safe, SEARCH_BASES[:3], 3)
    assert offs or safe, "a condition of the test: choose another top limb"
    assert limbs != 3 or offs, "a condition of the test: choose another top limb"
    got, surv = eng.prime_search(limbs, R.words(start, limbs), window, safe, np.array(SEARCH_BASES[:3], dtype=np.uint64), 3)
    assert (got.tolist(), surv) == (offs, survivors)
    # the sieve's survivors as candidates: every one carried to the top limb (offset 0 aside), and so did each half
    mask = R.sieve_mask(start, window, safe)
    surv_offs = [i for i in range(window) if mask[i]][:40]
    cs = [start + R.stride_of(safe) * i for i in surv_offs]
    assert all(c >> (64 * (limbs - 1)) == top + 1 for c, i in zip(cs, surv_offs) if i)
    _check(eng, limbs, cs + [(c - 1) // 2 for c in cs], SEARCH_BASES[:2])


def test_safe_search_from_a_start_with_bit_0_of_every_limb_set(eng):
    """the halving moves bit 0 of every limb into bit 63 of the limb below"""
    limbs = 3
    top = random.Random(0x7e10).getrandbits(62) | (1 << 61) | 1
    start = (top << 128) | (1 << 64) | 3
    assert all((start >> (64 * k)) & 1 for k in range(limbs)) and start % 4 == 3
    window = 1 << 15
    offs, survivors = R.search(start, window, True, SEARCH_BASES[:3], 3)
    assert offs, "a condition of the test: choose another top limb"
    got, surv = eng.prime_search(limbs, R.words(start, limbs), window, True, np.array(SEARCH_BASES[:3], dtype=np.uint64), 3)
    assert (got.tolist(), surv) == (offs, survivors)
