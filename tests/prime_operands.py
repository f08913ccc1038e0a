"""Structured operands for the prime generation's group arithmetic (csrc/prime_mont.cuh) and a model of it in Python integers
(DESIGN.md section 15.19).  The catalogue: shapes (limb count, bits in the top limb), modulus classes at a bit length, operands a below a
modulus, operands b below R, the pairs a test multiplies, triples found by search that reach states the classes do not, structured
primes, Proth primes with a quadratic non-residue, and small composites.  The model restates mont_mul, grp_sub, grp_double_mod and
prime_setup lane by lane -- the three-word columns, the one-limb move, the resolve step, the look-ahead as (G << 1) + P, the masked
subtraction -- and returns the states a product passed through.  Pure Python; the product must not import this module."""
import functools
import json
import os
import random
from typing import Dict, List, NamedTuple, Tuple

from tests import prime_ref as R

M64 = (1 << 64) - 1
TOP_BITS = (1, 2, 32, 33, 63, 64)
LIMBS_ALL = tuple(range(1, 33))
SHAPES = tuple((l, tb) for l in LIMBS_ALL for tb in TOP_BITS)
GROUP = 16
# the derivation of DESIGN.md 15.19: a column enters a step as lo + hi 2^64 with hi <= H, takes two products of at most (2^64 - 1)^2
# each and so holds at most 2^129 + (H - 3) 2^64 + 1: for H = 2 that is below 2^129, ex is at most 1, and the next hi = ex + (one carry)
# is at most 2 again
HI_BOUND = 2


def capacity(limbs: int) -> int:
    """E: limbs per lane of the kernel that takes `limbs`-limb candidates"""
    assert 1 <= limbs <= 32
    return 1 if limbs <= 16 else 2


def bits_of(limbs: int, tb: int) -> int:
    return 64 * (limbs - 1) + tb


def nwords(bits: int) -> int:
    return max(-(-bits // 64), 1)


def _rep(limb: int, bits: int) -> int:
    v = 0
    for j in range(nwords(bits)):
        v |= limb << (64 * j)
    return v & ((1 << bits) - 1)


def alt64(bits: int) -> int:
    v = 0
    for j in range(0, nwords(bits), 2):
        v |= M64 << (64 * j)
    return v & ((1 << bits) - 1)


# ---------------------------------------------------------------------------------------------------------------- the catalogue
CLASSES = ("all_ones", "pow2_plus1", "minus_2_64_plus1", "alt64", "hi32_1", "hi32_1_compl", "three", "2^64-59", "R-3", "random")


def moduli(limbs: int, tb: int) -> Dict[str, int]:
    """the modulus classes at b = 64 (limbs - 1) + tb bits, all odd and at least 3, by name.  3 and 2^64 - 59 (their upper limbs zero
    under a wide `limbs`) and R - 3 (the full capacity) come with tb = 64 only; a class that does not exist at b bits or repeats an
    earlier value is left out"""
    b = bits_of(limbs, tb)
    mask, top = (1 << b) - 1, 1 << (b - 1)
    rng = random.Random(0x7b33 + 131 * b)
    h = _rep(0xFFFFFFFF00000001, b)
    cand = [
        ("all_ones", mask),
        ("pow2_plus1", top + 1),
        ("minus_2_64_plus1", mask - (1 << 64) + 2 if b > 64 else 0),
        ("alt64", alt64(b) | top | 1),
        ("hi32_1", h | top | 1),
        ("hi32_1_compl", (~h & mask) | top | 1),
        ("three", 3 if tb == 64 else 0),
        ("2^64-59", (1 << 64) - 59 if tb == 64 else 0),
        ("R-3", (1 << (64 * limbs)) - 3 if tb == 64 else 0),
        ("random", rng.getrandbits(b) | top | 1),
    ]
    out: Dict[str, int] = {}
    for name, c in cand:
        small = name in ("three", "2^64-59")
        if c >= 3 and c & 1 and (small or c.bit_length() == b) and c not in out.values():
            out[name] = c
    return out


def operands_a(c: int, limbs: int) -> Dict[str, int]:
    """the first operand's classes, all below c; a value that repeats an earlier one goes by the earlier name"""
    Rr = 1 << (64 * limbs)
    E, bl = capacity(limbs), c.bit_length()
    rng = random.Random(0x7a11 + c % 1000003 + limbs)
    cand = [("0", 0), ("1", 1), ("2", 2), ("c-1", c - 1), ("c-2", c - 2), ("floor(c/2)", c // 2), ("ceil(c/2)", (c + 1) // 2), ("R mod c", Rr % c),
            ("R^2 mod c", Rr * Rr % c), ("(R-1) mod c", (Rr - 1) % c)]
    for j in range(E, limbs, E):                       # the lane boundaries
        cand += [("2^(64*%d-1)" % j, 1 << (64 * j - 1)), ("2^(64*%d)" % j, 1 << (64 * j))]
    cand += [("ones", (1 << (bl - 1)) - 1), ("alt64", alt64(bl - 1)), ("hi32", _rep(0xFFFFFFFF00000000, bl - 1)), ("lo32", _rep(0xFFFFFFFF, bl - 1)),
             ("random", rng.randrange(c))]
    out: Dict[str, int] = {}
    for name, v in cand:
        if 0 <= v < c and v not in out.values():
            out[name] = v
    return out


def operands_b(c: int, limbs: int) -> Dict[str, int]:
    """the scanned operand's classes: any value below R = 2^(64 limbs)"""
    Rr = 1 << (64 * limbs)
    rng = random.Random(0x7a22 + c % 1000003 + limbs)
    cand = [("0", 0), ("1", 1), ("R-1", Rr - 1), ("R-2", Rr - 2), ("R/2", Rr >> 1), ("c", c), ("c+1", c + 1), ("c-1", c - 1),
            ("lo32", _rep(0xFFFFFFFF, 64 * limbs)), ("hi32", _rep(0xFFFFFFFF00000000, 64 * limbs)), ("random", rng.getrandbits(64 * limbs))]
    out: Dict[str, int] = {}
    for name, v in cand:
        if 0 <= v < Rr and v not in out.values():
            out[name] = v
    return out


def pairs(c: int, limbs: int) -> List[Tuple[int, int]]:
    """the (a, b) a test multiplies under c: every a with two b (walking the b classes at two strides, so that every b class is met),
    and c - 1 with every b"""
    A, B = list(operands_a(c, limbs).values()), list(operands_b(c, limbs).values())
    out = []
    for i, a in enumerate(A):
        out += [(a, B[i % len(B)]), (a, B[(3 * i + 5) % len(B)])]
    out += [(c - 1, b) for b in B]
    return list(dict.fromkeys(out))


def triples(limbs: int) -> List[Tuple[str, int, int, int]]:
    """every (class @ top bits, a, b, c) of the catalogue at one limb count"""
    out = []
    for tb in TOP_BITS:
        for name, c in moduli(limbs, tb).items():
            out += [("%s@%d" % (name, tb), a, b, c) for a, b in pairs(c, limbs)]
    return out


# ---------------------------------------------------------------------------------------------------------------- the model
def _runs(P: int, recv: int) -> Tuple[int, int]:
    """(length, first lane) of the longest run of consecutive propagate lanes that received a carry; (0, -1) if none"""
    best, at, j = 0, -1, 0
    while j < GROUP:
        if (P >> j) & (recv >> j) & 1:
            k = j
            while k < GROUP and (P >> k) & (recv >> k) & 1:
                k += 1
            if k - j > best:
                best, at = k - j, j
            j = k
        else:
            j += 1
    return best, at


def carry_in(G: int, P: int) -> Tuple[int, int]:
    """grp_carry_in: the carries into the 16 lanes (a bit mask) and the carry out of lane 15, from the 17-bit addition (G << 1) + P"""
    assert G & P == 0 and G >> GROUP == 0 and P >> GROUP == 0, "a lane never generates and propagates"
    s = (G << 1) + P
    return (s ^ P) & 0xFFFF, (s >> 16) & 1


class SubState(NamedTuple):
    d: int             # a - b mod 2^(64 * 16 E)
    borrow: int        # the borrow out of lane 15 (a < b)
    run: int           # the longest run of propagate lanes that received a borrow
    start: int         # and the lane it started at


def sub_model(a: int, b: int, limbs: int) -> SubState:
    E = capacity(limbs)
    lw = 64 * E
    lm = (1 << lw) - 1
    G = P = 0
    d = [0] * GROUP
    for j in range(GROUP):
        x, y = (a >> (lw * j)) & lm, (b >> (lw * j)) & lm
        d[j] = (x - y) & lm
        G |= (x < y) << j
        P |= (d[j] == 0) << j
    bi, out = carry_in(G, P)
    v = 0
    for j in range(GROUP):
        v |= ((d[j] - ((bi >> j) & 1)) & lm) << (lw * j)
    assert v == (a - b) % (1 << (lw * GROUP)) and out == (a < b)
    return SubState(v, out, *_runs(P, bi))


def reduce_once_model(x: int, top: int, c: int, limbs: int) -> Tuple[int, bool, SubState]:
    """grp_reduce_once: x's low 16 E limbs, `top` the bit above them -> (x mod c, the subtraction was taken, its state)"""
    st = sub_model(x, c, limbs)
    take = bool(top) or not st.borrow
    return (st.d if take else x), take, st


class DoubleState(NamedTuple):
    r: int
    top: int           # the bit shifted out of lane 15
    taken: bool
    sub: SubState


def double_mod_model(x: int, c: int, limbs: int) -> DoubleState:
    assert 0 <= x < c
    W = 64 * GROUP * capacity(limbs)
    y, top = (x << 1) & ((1 << W) - 1), x >> (W - 1)
    r, taken, st = reduce_once_model(y, top, c, limbs)
    assert r == 2 * x % c
    return DoubleState(r, top, taken, st)


def setup_model(c: int, limbs: int) -> Tuple[int, int, int]:
    """prime_setup: (-c^-1 mod 2^64 by five Newton steps from x = c0, R mod c and R^2 mod c by 64 limbs doublings each)"""
    assert c & 1 and c >= 3
    m0 = c & M64
    x = m0
    for _ in range(5):
        x = x * (2 - m0 * x) & M64
    ninv = -x & M64
    assert (ninv * m0 + 1) & M64 == 0
    one = 1
    for _ in range(64 * limbs):
        one = double_mod_model(one, c, limbs).r
    r2 = one
    for _ in range(64 * limbs):
        r2 = double_mod_model(r2, c, limbs).r
    Rr = 1 << (64 * limbs)
    assert (one, r2) == (Rr % c, Rr * Rr % c)
    return ninv, one, r2


class MontState(NamedTuple):
    r: int
    lo: Tuple[int, ...]   # per limb after the last move
    hi: Tuple[int, ...]
    max_hi: int        # the largest hi after a move, over all steps and limbs
    max_ex: int        # the largest ex before a move
    out: int           # the look-ahead's carry out of lane 15
    top_hi: int        # the top limb's hi
    taken: bool        # the final subtraction was taken
    res_run: int       # resolve step: the longest run of propagate lanes that received a carry, and its first lane
    res_start: int
    sub_run: int       # the same in the final subtraction (borrows)
    sub_start: int
    borrow: int        # the final subtraction's borrow out of lane 15


def mont_mul_model(a: int, b: int, c: int, limbs: int) -> MontState:
    """mont_mul<E>(a, b, c, ninv, limbs): a < c, b < R = 2^(64 limbs), c odd.  Column k is one integer T[k] = lo + hi 2^64 + ex 2^128"""
    E = capacity(limbs)
    W = GROUP * E
    Rr = 1 << (64 * limbs)
    assert c & 1 and c >= 3 and 0 <= a < c < Rr and 0 <= b < Rr
    av, cv = [(a >> (64 * k)) & M64 for k in range(W)], [(c >> (64 * k)) & M64 for k in range(W)]
    ninv = -pow(c, -1, 1 << 64) & M64
    T = [0] * W
    V = max_hi = max_ex = 0
    for i in range(limbs):
        bi = (b >> (64 * i)) & M64
        m = ((T[0] + av[0] * bi) & M64) * ninv & M64
        T = [t + x * bi + y * m for t, x, y in zip(T, av, cv)]
        assert T[0] & M64 == 0
        max_ex = max(max_ex, max(T) >> 128)
        T = [(T[k] >> 64) + ((T[k + 1] & M64) if k + 1 < W else 0) for k in range(W)]       # one limb down
        max_hi = max(max_hi, max(T) >> 64)
        V = (V + a * bi + c * m) >> 64
        assert V < a + c, "the running value stays below a + c"
    assert max_hi <= HI_BOUND, "a column's hi is a count of at most 2"
    lo, hi = [t & M64 for t in T], [t >> 64 for t in T]
    assert sum(l << (64 * k) for k, l in enumerate(lo)) + sum(h << (64 * (k + 1)) for k, h in enumerate(hi)) == V
    # resolve: lane j's limbs take the hi below them; per lane a carry (generate) or all ones (propagate)
    lw = 64 * E
    lm = (1 << lw) - 1
    G = P = 0
    lane = [0] * GROUP
    for j in range(GROUP):
        t = sum((lo[j * E + e] + (hi[j * E + e - 1] if j * E + e else 0)) << (64 * e) for e in range(E))
        lane[j] = t & lm
        # a limb wraps only by taking a hi of at most 2 (or a carry), which leaves at most 1: a lane that carries is never all ones, so
        # the kernel's `ones && cy == 0` equals `ones`
        assert not (t >> lw and t & lm == lm)
        G |= (t >> lw) << j
        P |= (t == lm) << j
    assert max(G, P) >> GROUP == 0
    ci, out = carry_in(G, P)
    x = 0
    for j in range(GROUP):
        x |= ((lane[j] + ((ci >> j) & 1)) & lm) << (lw * j)
    top_hi = hi[W - 1]
    assert x + ((out + top_hi) << (lw * GROUP)) == V and out + top_hi <= 1, "one bit above the group's width is all that remains"
    r, taken, st = reduce_once_model(x, out or top_hi, c, limbs)
    assert r == a * b * pow(Rr, -1, c) % c
    res_run, res_start = _runs(P, ci)
    return MontState(r, tuple(lo), tuple(hi), max_hi, max_ex, out, top_hi, taken, res_run, res_start, st.run, st.start, st.borrow)


def state_key(s: MontState) -> Tuple:
    """what the state table pins per modulus class: (largest hi, out, top_hi, subtraction taken, borrow left lane 15, resolve run, subtraction run)"""
    return (s.max_hi, s.out, s.top_hi, int(s.taken), s.borrow, min(s.res_run, 3), min(s.sub_run, 3))


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _golden(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


PATTERNS = ("all_ones", "pow2_plus1", "minus_2_64_plus1", "alt64", "hi32_1", "hi32_1_compl", "R-3")


def pattern(name: str, limbs: int) -> int:
    """a modulus class at full width (64 limbs bits)"""
    return moduli(limbs, 64)[name]


def pattern_prime(limbs: int, name: str, k: int, sign: int) -> int:
    return pattern(name, limbs) + sign * 2 * k


@functools.lru_cache(maxsize=None)
def structured_primes() -> List[Tuple[int, str, int, int]]:
    """[(limbs, pattern, k, sign)]: pattern + sign 2 k is prime with exactly 64 limbs bits, k the smallest such (the sign that stays at
    the width: minus for the patterns at the top of the range, plus for 2^(b-1) + 1)"""
    return [tuple(e) for e in _golden("structured_prime_patterns.json")["patterns"]]


@functools.lru_cache(maxsize=None)
def proth_primes() -> List[Tuple[int, int, int]]:
    """[(s, k, z)]: k 2^s + 1 prime with the smallest odd k, z a small quadratic non-residue (Jacobi symbol -1)"""
    return [tuple(e) for e in _golden("structured_prime_patterns.json")["proth"]]


def jacobi(a: int, n: int) -> int:
    assert n > 0 and n & 1
    a %= n
    r = 1
    while a:
        while a % 2 == 0:
            a //= 2
            if n % 8 in (3, 5):
                r = -r
        a, n = n, a
        if a % 4 == 3 and n % 4 == 3:
            r = -r
        a %= n
    return r if n == 1 else 0


def first_minus_one(c: int, base: int) -> int:
    """the number of squarings of base^d (c - 1 = d 2^s) after which the value first is c - 1; -1 if never within s - 1"""
    d, s = c - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    y = pow(base, d, c)
    for i in range(s):
        if y == c - 1:
            return i
        y = y * y % c
    return -1


# small composites: 341 is a Fermat pseudoprime to base 2 that no -1 precedes; the Carmichael numbers pass a^(c-1) = 1 for every
# coprime base.  A brute-force search over every odd composite c below 2^20 and every base 1 < a < c for a^(c-1) = -1 (mod c) -- the
# one kind of value that would tell `pos >= 1` from `pos >= 0` in k_prime_mr's window -- finds none, and none exists at all: a^(c-1) =
# -1 mod c gives a an order 2^(t+1) k modulo every prime factor p of c, where 2^t is the power of two in c - 1; then 2^(t+1) divides
# p - 1 for every p, so c = 1 mod 2^(t+1), which contradicts the choice of t.  tests/golden/make_structured_primes.py runs the search.
SMALL_NEGATIVES = (341, 1105, 1729, 2465, 6601)
MINUS_ONE_AT_POS_0_BELOW_2_20 = ()

# bases of the structured-prime runs: the fifteen prime bases and six with structured limbs
STRUCT_BASES = R.PRIME_BASES + (1 << 63, (1 << 64) - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 0xFFFFFFFF00000000)


# ---------------------------------------------------------------------------------------------------------------- searched triples
# Found by tests/golden/make_structured_primes.py with the model: (limbs, modulus class at full width, seed, (m, sh)) stands for
# a = Random(seed).randrange(1, c) and b = a^-1 R target mod c with target = m 2^sh (m > 0) or c + m (m < 0), so that the product is
# `target` and the value before the final subtraction is target or target + c.  What each reaches is pinned beside it: (out, top_hi, resolve run, its first lane, subtraction
# run, its first lane).  `out = 1` needs the full capacity (16 or 32 limbs) and a c near R; a run of propagate lanes that receive a carry
# needs limbs of the value that are zero, which random residues never have.
SEARCHED: Tuple[Tuple[int, str, int, Tuple[int, int], Tuple[int, int, int, int, int, int]], ...] = (
    (16, "R-3", 0, (3, 0), (1, 0, 14, 2, 0, -1)),              # out, behind a carry that ripples from lane 2 through lane 15
    (16, "R-3", 0, (-1, 0), (0, 0, 0, -1, 15, 1)),             # a borrow from lane 0 through every lane, and out of lane 15
    (16, "R-3", 2, (1, 960), (1, 0, 0, -1, 0, -1)),            # out generated in lane 15 itself
    (16, "pow2_plus1", 0, (1, 192), (0, 0, 10, 5, 0, -1)),     # a carry ripple that starts and ends inside the group
    (32, "R-3", 0, (3, 0), (1, 0, 15, 1, 0, -1)),
    (32, "R-3", 0, (-1, 0), (0, 0, 0, -1, 15, 1)),
    (32, "R-3", 3, (1, 1984), (1, 0, 0, -1, 0, -1)),
    (32, "pow2_plus1", 0, (1, 384), (0, 0, 11, 4, 0, -1)),
    (8, "R-3", 0, (3, 0), (0, 0, 6, 2, 0, -1)),                # narrower than the group: the ripple ends where the value does
    (8, "R-3", 0, (-1, 0), (0, 0, 0, -1, 15, 1)),              # the borrow crosses the zero lanes above the value
    (8, "R-3", 2, (1, 256), (0, 0, 3, 5, 0, -1)),
    (17, "R-3", 0, (3, 0), (0, 0, 7, 1, 0, -1)),
    (17, "R-3", 0, (-1, 0), (0, 0, 0, -1, 15, 1)),
    (17, "R-3", 0, (1, 512), (0, 0, 3, 5, 0, -1)),
)


def searched_triple(limbs: int, cls: str, seed: int, target: Tuple[int, int]) -> Tuple[int, int, int]:
    c = pattern(cls, limbs)
    target = target[0] << target[1] if target[0] > 0 else c + target[0]
    assert 0 < target < c
    a = random.Random(seed).randrange(1, c)
    while True:
        try:
            b = pow(a, -1, c) * (1 << (64 * limbs)) * target % c
            return a, b, c
        except ValueError:          # a shares a factor with c: the next value
            a += 1


def searched_state(s: MontState) -> Tuple[int, int, int, int, int, int]:
    return (s.out, s.top_hi, s.res_run, s.res_start, s.sub_run, s.sub_start)
