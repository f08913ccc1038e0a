"""Structured operands for the big-integer kernels (K3, csrc/pz_bigint.hip) and a model of the device's mul_mod in Python integers
(DESIGN.md section 15.13).  The catalogue: shapes (limb count, bits in the top limb), modulus classes at a bit length, operand
classes below a modulus, the pairs a test multiplies, Mersenne and structured-prime keys.  The model restates Barrett's estimate as
pz_bigint.hip computes it -- the normalised modulus, the reciprocal with its clamp, qhat, the corrections and the limb above the
capacity at loop entry -- and the path the normalisation shift takes.  Pure Python; the product must not import this module."""
import functools
import json
import math
import os
import random
from typing import Dict, List, NamedTuple, Tuple

M64 = (1 << 64) - 1
TOP_BITS = (1, 2, 32, 33, 63, 64)
LN_E1 = (1, 8, 9, 16, 24, 31, 32)
LN_E2 = (33, 48, 49, 64)
LN_ALL = LN_E1 + LN_E2
L_ALL = tuple(2 * ln for ln in LN_ALL)          # 2, 16, 18, 32, 48, 62, 64 | 66, 96, 98, 128
SHAPES_N = tuple((ln, tb) for ln in LN_ALL for tb in TOP_BITS)        # n has ln limbs; the modulus is n^2 in 2 ln limbs
SHAPES_M = tuple((l, tb) for l in L_ALL for tb in TOP_BITS)           # the modulus itself has l limbs

MERSENNE = ((61, 89), (89, 107), (107, 127), (127, 521), (521, 607), (607, 1279), (1279, 2203))
MERSENNE_BITS = (150, 196, 234, 648, 1128, 1886, 3482)


def bits_of(limbs: int, tb: int) -> int:
    return 64 * (limbs - 1) + tb


def words(bits: int) -> int:
    return max(-(-bits // 64), 1)


def capacity(limbs: int) -> int:
    """E: limbs per lane of the kernel that takes `limbs`-limb operands"""
    assert 1 <= limbs <= 128
    return 1 if limbs <= 64 else 2


def slice_limbs(limbs: int) -> int:
    """limbs of the first operand one wave of a team multiplies: 16 at E = 1, 32 at E = 2"""
    return 16 * capacity(limbs)


def _rep(limb: int, bits: int) -> int:
    v = 0
    for j in range(words(bits)):
        v |= limb << (64 * j)
    return v & ((1 << bits) - 1)


def alt64(bits: int) -> int:
    """limbs alternating all ones / zero, from limb 0"""
    v = 0
    for j in range(0, words(bits), 2):
        v |= M64 << (64 * j)
    return v & ((1 << bits) - 1)


def alt32_hi(bits: int) -> int:
    return _rep(0xFFFFFFFF00000000, bits)


def alt32_lo(bits: int) -> int:
    return _rep(0x00000000FFFFFFFF, bits)


def moduli(b: int, seed: int = 0) -> Dict[str, int]:
    """the modulus classes at exactly b bits, by name; a class that does not exist at b bits, or repeats an earlier one, is left out"""
    top = 1 << (b - 1)
    rng = random.Random(0x6b33 + 131 * b + seed)
    cand = [
        ("all_ones", (1 << b) - 1),
        ("pow2_plus1", top + 1),
        ("pow2", top),
        ("minus_2_64_plus1", (1 << b) - (1 << 64) + 1 if b > 64 else 0),
        ("alt64", alt64(b) | top | 1),
        ("alt32_hi", alt32_hi(b) | top | 1),
        ("alt32_lo", alt32_lo(b) | top | 1),
        ("random", rng.getrandbits(b) | top | 1),
    ]
    out: Dict[str, int] = {}
    for name, m in cand:
        if m > 0 and m.bit_length() == b and m not in out.values():
            out[name] = m
    return out


def odd_only(ms: Dict[str, int]) -> Dict[str, int]:
    """the odd moduli above 1 (what pz_bigint_mod_inverse takes)"""
    return {k: m for k, m in ms.items() if m & 1 and m > 1}


def _candidates(m: int, limbs: int, n: int = 0) -> List[Tuple[str, int]]:
    bl = m.bit_length()
    r = math.isqrt(m)
    cand = [("0", 0), ("1", 1), ("2", 2), ("m-1", m - 1), ("m-2", m - 2), ("floor(m/2)", m // 2), ("ceil(m/2)", (m + 1) // 2),
            ("isqrt", r), ("isqrt+1", r + 1), ("ones", (1 << (bl - 1)) - 1), ("alt64", alt64(bl - 1)), ("alt32_hi", alt32_hi(bl - 1)),
            ("alt32_lo", alt32_lo(bl - 1))]
    for j in range(slice_limbs(limbs), limbs, slice_limbs(limbs)):
        cand += [("2^(64*%d-1)" % j, 1 << (64 * j - 1)), ("2^(64*%d)" % j, 1 << (64 * j))]
    cand += [("2^top", 1 << (bl - 1)), ("2^(top-1)", 1 << max(bl - 2, 0)), ("m-2^(top-1)", m - (1 << max(bl - 2, 0)))]
    if n:
        assert m == n * n
        cand += [("n", n), ("3n", 3 * n), ("n*ones63", n * ((1 << 63) - 1) if n >> 63 else 0), ("n+1", n + 1), ("1+(n-1)n", 1 + (n - 1) * n),
                 ("(n-1)n", (n - 1) * n)]
    return [(name, v) for name, v in cand if 0 <= v < m]


def operands(m: int, limbs: int, n: int = 0) -> Dict[str, int]:
    """the operand classes below m, by name (m = n^2 if n is given); a value that is not below m is left out, and one that repeats an
    earlier one goes by the earlier name (under n^2, isqrt is n)"""
    out: Dict[str, int] = {}
    for name, v in _candidates(m, limbs, n):
        if v not in out.values():
            out[name] = v
    return out


def by_name(m: int, limbs: int, n: int = 0) -> Dict[str, int]:
    """every class that exists under m by its own name, repeated values included (a test that picks a few classes by name)"""
    return dict(_candidates(m, limbs, n))


def pairs(m: int, limbs: int, n: int = 0) -> List[Tuple[str, str]]:
    """the (a, b) classes a test multiplies, by the names operands() gives: the fixed ones, every class with its successor in the
    catalogue's order, a few squares, and for m = n^2 the pairs with r = 0 (q = 1, 3, 2^63 - 1, x y = 9 and 3 (2^63 - 1), (n - 1)^2) -- only
    over classes that exist under m"""
    ops = operands(m, limbs, n)
    first = {v: name for name, v in reversed(list(ops.items()))}
    alias = {name: first[v] for name, v in _candidates(m, limbs, n)}
    names = list(ops)
    want = [("m-1", "m-1"), ("m-1", "1"), ("1", "m-1"), ("isqrt+1", "isqrt+1"), ("isqrt", "isqrt"), ("isqrt", "isqrt+1"), ("m-2", "m-2"),
            ("ones", "ones"), ("alt32_hi", "alt32_hi"), ("alt32_lo", "alt32_hi"), ("alt64", "alt64"), ("2^top", "2^top"), ("m-1", "0"),
            ("m-1", "m-2"), ("floor(m/2)", "2"), ("ceil(m/2)", "2"), ("m-1", "m-2^(top-1)"), ("m-2^(top-1)", "m-2")]
    if n:
        want += [("n", "n"), ("n", "3n"), ("3n", "n"), ("(n-1)n", "(n-1)n"), ("n+1", "1+(n-1)n"), ("1+(n-1)n", "1+(n-1)n"), ("n", "n*ones63"),
                 ("3n", "3n"), ("3n", "n*ones63")]
    want += [(a, names[(i + 1) % len(names)]) for i, a in enumerate(names)]
    out = []
    for a, b in want:
        if a in alias and b in alias and (alias[a], alias[b]) not in out:
            out.append((alias[a], alias[b]))
    return out


def unreduced(m: int, limbs: int) -> Dict[str, int]:
    """operands of `limbs` limbs that need not be below m (pz_mul_mod takes them): the quotient may or may not fit `limbs` limbs"""
    full = (1 << (64 * limbs)) - 1
    return {"full": full, "2^(64L-1)": 1 << (64 * limbs - 1), "m": m, "m+1": min(m + 1, full), "2m-1": min(2 * m - 1, full), "1": 1, "2": 2}


UNREDUCED_PAIRS = (("full", "full"), ("full", "1"), ("full", "2"), ("2^(64L-1)", "2"), ("m", "m"), ("m+1", "m+1"), ("2m-1", "2m-1"),
                   ("full", "m"), ("2^(64L-1)", "2^(64L-1)"))


# ---------------------------------------------------------------------------------------------------------------- the model
class Model(NamedTuple):
    E: int
    ls: int            # the normalisation shift: whole limbs
    bs: int            # and bits
    clamp: bool        # the reciprocal was clamped (M' = 2^(N - 1))
    qhat: int
    corrections: int
    top: int           # the limb above the capacity of y - qhat M' at loop entry
    q: int
    r: int
    lost: bool         # the quotient does not fit the capacity (the device's ST_RANGE before ld_exceeds)


@functools.lru_cache(maxsize=4096)
def barrett(m: int, limbs: int):
    """(E, N, s, M', mu) as barrett_setup computes them"""
    E = capacity(limbs)
    N = 4096 * E
    assert 0 < m < 1 << (64 * limbs)
    s = N - m.bit_length()
    M = m << s
    if M == 1 << (N - 1):
        mu = (1 << N) - 1                        # floor(2^N (2^N - M') / M') would be 2^N: clamped
    else:
        mu = ((1 << N) - M << N) // M
        assert mu == (1 << (2 * N)) // M - (1 << N) and mu < 1 << N
    return E, N, s, M, mu


def mul_mod_model(a: int, b: int, m: int, limbs: int) -> Model:
    E, N, s, M, mu = barrett(m, limbs)
    y = (a * b) << s
    lost = y >> (2 * N) != 0
    y &= (1 << (2 * N)) - 1
    yhi, ylo = y >> N, y & ((1 << N) - 1)
    qhat = yhi + (yhi * mu >> N)
    if qhat >> N:
        lost = True
    if lost:
        return Model(E, s >> 6, s & 63, M == 1 << (N - 1), qhat, 0, 0, a * b // m, a * b % m, True)
    rem = y - qhat * M
    assert rem >= 0, "the estimate never exceeds the quotient"
    z = qhat * M
    borrow = 1 if ylo < (z & ((1 << N) - 1)) else 0
    top = ((yhi & M64) - ((z >> N) & M64) - borrow) & M64
    assert top == rem >> N, "one limb above the capacity holds what is left"
    corrections = rem // M
    q, r = qhat + corrections, (rem - corrections * M) >> s
    assert (q, r) == divmod(a * b, m) and (rem - corrections * M) & ((1 << s) - 1) == 0
    return Model(E, s >> 6, s & 63, M == 1 << (N - 1), qhat, corrections, top, q, r, False)


def shift_path(E: int, ls: int, bs: int) -> str:
    """the branch shl_2c / shr_c take"""
    if E == 1 and ls == 0:
        return "dpp bs=0" if bs == 0 else "dpp bs=1" if bs == 1 else "dpp bs>=62" if bs >= 62 else "dpp"
    if E == 1:
        return ("lds ls=1" if ls == 1 else "lds ls>=2") + (" bs=0" if bs == 0 else " bs!=0")
    return ("lds E=2 ls=0" if ls == 0 else "lds E=2 ls>=1") + (" bs=0" if bs == 0 else " bs!=0")


# ---------------------------------------------------------------------------------------------------------------- keys
def mersenne_primes(i: int) -> Tuple[int, int]:
    a, b = MERSENNE[i]
    return (1 << a) - 1, (1 << b) - 1


def structured_primes() -> Dict[str, Dict[str, int]]:
    """tests/golden/structured_primes.json: per k the smallest c with 2^k - c prime, the next one, and the smallest c' with
    2^(k-1) + c' prime"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "structured_primes.json")) as f:
        return json.load(f)


def structured_key_primes(which: str) -> Tuple[int, int]:
    """'mixed': (2^1024 - c1)(2^1023 + c_low): n = 2^2047 + (a run of zeros) + ..., n^2 has 4095 bits (the DPP shift by one bit);
    'high': (2^1024 - c1)(2^1024 - c2): n = 2^2048 - (c1 + c2) 2^1024 + c1 c2, n^2 has 4096 bits (no shift).  Both n have 2048 bits."""
    d = structured_primes()["1024"]
    p = (1 << 1024) - d["c1"]
    assert which in ("mixed", "high")
    return (p, (1 << 1023) + d["c_low"]) if which == "mixed" else (p, (1 << 1024) - d["c2"])


STRUCTURED_KEYS = ("mixed", "high")


def general_g(n: int, lam: int, seed: int) -> int:
    """a non-standard g below n whose order n divides, found as tests/decrypt_ref.key finds it"""
    rng = random.Random(0x6e6 + seed)
    while True:
        g = rng.randrange(2, n)
        u = pow(g, lam, n * n)
        if math.gcd(g, n) == 1 and u % n == 1 and math.gcd(u // n, n) == 1:
            return g


def full_key(p: int, q: int, g: int = 0):
    """(n, g, lam, d, mu, ginv) as tests/decrypt_ref.key returns it, for any two primes"""
    n = p * q
    lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    g = g or n + 1
    x = pow(g, lam, n * n) // n
    return n, g, lam, pow(n, -1, lam), pow(x, -1, n), pow(g, -1, n)
