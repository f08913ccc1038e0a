"""Python-integer models of the device prime generation (pz.h pz_bigint_is_prime, pz_prime_sieve,
pz_prime_search) and the catalogue of candidates the CPU and GPU tests share, every entry with its pinned witness index."""
import json
import os

MASK64 = (1 << 64) - 1
NO_ROUND = 0xFFFFFFFF
# the catalogue's bases: the primes 2 .. 47
PRIME_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47)
ALL_PASS = len(PRIME_BASES)


def mr_first_witness(c, bases):
    """-> (flag, witness) exactly as pz_bigint_is_prime reports one candidate: c < 2 or an even c > 2: (0, 0xFFFFFFFF); c = 2:
    (1, 0xFFFFFFFF); otherwise, with c - 1 = d 2^s and a = bases[k] mod c, round k passes if a is 0, 1 or c - 1, else if a^d is 1 or
    c - 1, else if one of the next s - 1 squarings gives c - 1; witness = the first failing round, len(bases) if none fails."""
    if c < 2 or (c > 2 and c % 2 == 0):
        return 0, NO_ROUND
    if c == 2:
        return 1, NO_ROUND
    d, s = c - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for k, b in enumerate(bases):
        a = b % c
        if a in (0, 1, c - 1):
            continue
        y = pow(a, d, c)
        if y in (1, c - 1):
            continue
        for _ in range(s - 1):
            y = y * y % c
            if y == c - 1:
                break
        else:
            return 0, k
    return 1, len(bases)


def _odd_primes_below(limit):
    comp = bytearray(limit)
    out = []
    for p in range(3, limit, 2):
        if not comp[p]:
            out.append(p)
            for q in range(p * p, limit, 2 * p):
                comp[q] = 1
    return out


SIEVE_PRIMES = _odd_primes_below(1 << 16)
assert len(SIEVE_PRIMES) == 6541


def stride_of(safe):
    return 4 if safe else 2


def sieve_mask(start, window, safe):
    """mask[i] = 1 iff no odd prime p below 2^16 divides c_i = start + stride i, nor -- with safe -- (c_i - 1) / 2, i.e. c_i != 1 mod p"""
    stride = stride_of(safe)
    mask = bytearray(b"\x01") * window
    for p in SIEVE_PRIMES:
        r = start % p
        inv = pow(stride, -1, p)
        for target in ((0, 1) if safe else (0,)):
            for i in range((target - r) * inv % p, window, p):
                mask[i] = 0
    return bytes(mask)


def search(start, window, safe, bases, want):
    """-> (offsets, survivors): the `want` smallest offsets whose c_i survives the sieve and passes every round (with safe, whose
    (c_i - 1) / 2 passes too), and the sieve's survivor count"""
    stride = stride_of(safe)
    mask = sieve_mask(start, window, safe)
    out = []
    for i in range(window):
        if len(out) == want:
            break
        if not mask[i]:
            continue
        c = start + stride * i
        if mr_first_witness(c, bases)[0] and (not safe or mr_first_witness((c - 1) // 2, bases)[0]):
            out.append(i)
    return out, sum(mask)


def words(x, limbs):
    assert 0 <= x < 1 << (64 * limbs)
    return [(x >> (64 * i)) & MASK64 for i in range(limbs)]


def golden_primes():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paillier_keys.json")
    keys = json.load(open(path))
    return {int(b): (int(kv["p"], 16), int(kv["q"], 16)) for b, kv in keys.items()}


def _catalogue():
    """[(name, value, witness index against PRIME_BASES)]: every index pinned here, checked again by tests/test_keygen.py"""
    P = ALL_PASS
    out = [
        # strong pseudoprimes: each passes every base before its first failing one
        ("psp 561", 561, 0),
        ("psp 3215031751", 3215031751, 4),
        ("psp 3825123056546413051", 3825123056546413051, 11),
        ("psp 318665857834031151167461", 318665857834031151167461, 12),
        ("psp 3317044064679887385961981", 3317044064679887385961981, 13),
    ]
    # primes at the top of the capacity and their neighbours (the neighbour above 2^e - k stays below 2^e: k > 2)
    for e, k in ((64, 59), (128, 159), (256, 189), (512, 569), (1024, 105), (2048, 1557)):
        out += [("2^%d-%d" % (e, k), 2 ** e - k, P), ("2^%d-%d" % (e, k + 2), 2 ** e - k - 2, 0), ("2^%d-%d" % (e, k - 2), 2 ** e - k + 2, 0)]
    for e in (61, 89, 107, 127, 521, 607, 1279):
        out.append(("M%d" % e, 2 ** e - 1, P))
    # long runs of trailing zeros in c - 1 across limb boundaries: k 2^s + 1, primes and the composites next to them
    for k, s, wit in ((9, 63, P), (7, 63, 0), (11, 63, 0), (25, 64, P), (23, 64, 0), (27, 64, P), (9, 65, P), (7, 65, 0), (11, 65, 0),
                      (205, 130, P), (203, 130, 0), (207, 130, P), (13, 1000, P), (11, 1000, 0), (15, 1000, 0)):
        out.append(("%d*2^%d+1" % (k, s), k * 2 ** s + 1, wit))
    # products of two primes and squares of primes from the golden keys (n up to 2048 bits), and small squares
    for bits, (p, q) in sorted(golden_primes().items()):
        if bits <= 2048:
            out += [("golden n %d" % bits, p * q, 0), ("golden p^2 %d" % bits, p * p, 0), ("golden p %d" % bits, p, P), ("golden q %d" % bits, q, P)]
    out += [("3^2", 9, 0), ("5^2", 25, 0), ("65521^2", 65521 ** 2, 0), ("(2^61-1)^2", (2 ** 61 - 1) ** 2, 0), ("(2^64-59)^2", (2 ** 64 - 59) ** 2, 0)]
    # the small ends of the definition
    out += [("0", 0, NO_ROUND), ("1", 1, NO_ROUND), ("2", 2, NO_ROUND), ("3", 3, P), ("4", 4, NO_ROUND), ("5", 5, P), ("2^64-2", 2 ** 64 - 2, NO_ROUND),
            ("2^64-1", 2 ** 64 - 1, 0), ("F6 = 2^64+1", 2 ** 64 + 1, 1), ("2^64+13", 2 ** 64 + 13, P), ("2^1024", 2 ** 1024, NO_ROUND)]
    return out


CATALOGUE = _catalogue()

# bases that reduce to 0, 1 and c - 1 pass their round: (value, bases, witness)
REDUCING = [
    (47, (47, 48, 46, 94, 2 ** 64 - 21), 5),         # 2^64 - 21 = 3 mod 47: an ordinary round, and 47 is prime
    (15, (15, 16, 14, 30, 31, 29, 2), 6),             # 0, 1, -1, 0, 1, -1 pass; 2 fails
    (2 ** 64 - 59, (2 ** 64 - 59, 2 ** 64 - 58, 2 ** 64 - 60, 2), 4),
    (2 ** 61 - 1, (2 ** 61 - 1, 2 ** 61, 2 ** 61 - 2, 2 ** 62 - 2, 3), 5),
    (25 * 2 ** 64 + 1, (2 ** 64 - 1, 2), 2),
    (9, (9, 10, 8, 18, 2), 4),
]


def fits(c, limbs):
    return c < 1 << (64 * limbs)
