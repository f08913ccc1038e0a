"""Paillier secret keys as Python integers: what Engine.paillier_sk (pz.h pz_paillier_sk_create) takes, and the dealer of a T-of-T
threshold key (deal_shares): additive shares of the decryption exponent for Engine.paillier_partial and the
public ThresholdKey for Engine.paillier_combine and the verifier of circuit kind 'partial'; and of a t-of-T key (deal_shamir,
lagrange_exponents; section 15.12): Shamir shares for the same Engine.paillier_partial and the public ShamirKey for
Engine.paillier_combine_t; and the generator of the primes all of them start from (is_probable_prime, generate_prime, generate_key;
section 15.16), which runs on the device: Engine.is_prime and Engine.prime_search.

The library derives mu and g^-1 on the device and validates the key there; the one value it does not derive is d = n^-1 mod lambda,
the exponent that recovers an encryption's randomness: it is the caller's, and this helper computes it.
A handle that also decrypts by the CRT (Engine.paillier_sk(limbs_n, n, g, lam, d, p, q); pz.h pz_paillier_sk_create_crt; section 15.22)
takes six values: the four of secret_from_primes(p, q, g) and the primes p and q themselves, in either order.
djn_generator makes the element hs that short-randomness ("DJN mode") encryption adds to a public key (section 15.18).
pack_choices, unpack_tally, pballot_capacity and pballot_bases serve the packed ballot, K choices in one ciphertext (section 15.21)."""
from __future__ import annotations

import math
import secrets
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple


def secret_from_primes(p: int, q: int, g: Optional[int] = None) -> Tuple[int, int, int, int]:
    """(n, g, lam, d) of the key with primes p and q: n = p q, lam = lcm(p - 1, q - 1), d = n^-1 mod lam; g defaults to n + 1.
    Needs gcd(n, (p - 1)(q - 1)) = 1 (true of any two primes of one length), else n has no inverse mod lam: ValueError.
    A general g must have an order n divides (g^lam mod n^2 = 1 + x n with x a unit mod n): ValueError otherwise."""
    if p < 3 or q < 3 or p == q:
        raise ValueError("p and q must be distinct odd primes")
    n = p * q
    if math.gcd(n, (p - 1) * (q - 1)) != 1:
        raise ValueError("gcd(n, phi(n)) != 1: n has no inverse mod lambda")
    lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    if g is None:
        g = n + 1
    u = pow(g, lam, n * n)
    if not 0 < g < n * n or u % n != 1 or math.gcd(u // n, n) != 1:
        raise ValueError("n does not divide the order of g")
    return n, g, lam, pow(n, -1, lam)


# ---------------------------------------------------------------------------------------------------------------------------------
# T-of-T threshold keys: a dealer splits theta = lam (lam^-1 mod n) additively among the trustees
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_TRUSTEES = 256


@dataclass(frozen=True)
class ThresholdKey:
    """the PUBLIC threshold key: hs[i] = v^theta_i mod n^2 is what trustee i's proofs (circuit kind 'partial') are checked against,
    mu2 = (2a)^-1 mod n with 1 + a n = g^theta mod n^2 is the combiner's last factor.  v_order_proved: the dealer checked that v has
    order n lam / 2, the exponent of the squares mod n^2 -- only then does a verified proof pin the partial for EVERY ciphertext."""
    n: int
    g: int
    v: int
    hs: Tuple[int, ...]
    mu2: int
    v_order_proved: bool


def _is_prime(x: int) -> bool:
    """Miller-Rabin over the first twelve primes (deterministic below 318665857834031151167461, the least strong pseudoprime to all
    twelve) and 24 more fixed bases from there on"""
    if x < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for s in small:
        if x % s == 0:
            return x == s
    d, r = x - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    bases = small if x < 318665857834031151167461 else small + tuple(range(41, 137, 4))
    for a in bases:
        y = pow(a, d, x)
        if y in (1, x - 1):
            continue
        for _ in range(r - 1):
            y = y * y % x
            if y == x - 1:
                break
        else:
            return False
    return True


def deal_shares(p: int, q: int, trustees: int, g: Optional[int] = None,
                rand: Callable[[int], int] = secrets.randbelow) -> Tuple[ThresholdKey, List[int]]:
    """The dealer: (public ThresholdKey, [theta_1 .. theta_T]) for the key with primes p and q.  theta = lam (lam^-1 mod n), so theta = 0
    mod lam and 1 mod n; theta_1 .. theta_{T-1} = rand(n lam) each (rand(k): uniform in [0, k), by default secrets.randbelow) and
    theta_T = (theta - their sum) mod n lam: every share is non-negative and below n^2, any T - 1 of them are independent uniform values.
    v = w^2 mod n^2 for a w drawn with rand.  With safe primes ((p - 1) / 2 and (q - 1) / 2 prime) v is resampled until its order is
    n lam / 2: v^(N/2) = 1 and v^((N/2)/l) != 1 for l in {p, q, (p - 1) / 2, (q - 1) / 2}; for other primes the factors of lam / 2 are
    unknown, the first unit's square is taken and v_order_proved is False.  Refuses what secret_from_primes refuses, and trustees
    outside 1 .. 256: ValueError.  The dealer must forget p, q, lam, theta and the shares it hands out."""
    n, g, lam, _ = secret_from_primes(p, q, g)
    if isinstance(trustees, bool) or not isinstance(trustees, int) or not 1 <= trustees <= MAX_TRUSTEES:
        raise ValueError(f"trustees must be 1 .. {MAX_TRUSTEES}, not {trustees!r}")
    n2, N = n * n, n * lam
    theta = lam * pow(lam, -1, n)
    shares = [rand(N) for _ in range(trustees - 1)]
    shares.append((theta - sum(shares)) % N)
    pp, qq = (p - 1) // 2, (q - 1) // 2
    safe = _is_prime(pp) and _is_prime(qq) and pp != qq
    half = N // 2            # = n pp qq for safe primes
    while True:
        w = rand(n2)
        if w < 2 or math.gcd(w, n) != 1:
            continue
        v = w * w % n2
        if v == 1:
            continue
        if not safe or (pow(v, half, n2) == 1 and all(pow(v, half // l, n2) != 1 for l in (p, q, pp, qq))):
            break
    a = (pow(g, theta, n2) - 1) // n
    key = ThresholdKey(n=n, g=g, v=v, hs=tuple(pow(v, s, n2) for s in shares), mu2=pow(2 * a, -1, n), v_order_proved=safe)
    return key, shares


# ---------------------------------------------------------------------------------------------------------------------------------
# t-of-T threshold keys: the dealer shares theta by a polynomial of degree t - 1 over Z_(n lam)
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ShamirKey:
    """the PUBLIC t-of-T key: hs[i - 1] = v^(s_i) mod n^2 is what trustee i's proofs (circuit kind 'partial') are checked against, as
    with a ThresholdKey; mu2 = (2 a trustees!)^-1 mod n with 1 + a n = g^theta mod n^2 is the last factor of Engine.paillier_combine_t
    over any `threshold` of the `trustees` partials.  v_order_proved as in ThresholdKey."""
    n: int
    g: int
    v: int
    hs: Tuple[int, ...]
    mu2: int
    trustees: int
    threshold: int
    v_order_proved: bool


def lagrange_exponents(trustees: int, ids) -> List[int]:
    """mu_i = trustees! * prod_{j in ids, j != i} j / (j - i) for every i of ids, in their order, as signed integers (each IS an integer:
    asserted).  sum_i mu_i f(i) = trustees! f(0) for every polynomial f of degree below len(ids).  ids: distinct, 1 .. trustees <= 256:
    ValueError otherwise.  (pz.h pz_shamir_lagrange is the same in C; this restates it independently in Python integers.)"""
    ids = list(ids)
    if isinstance(trustees, bool) or not isinstance(trustees, int) or not 1 <= trustees <= MAX_TRUSTEES:
        raise ValueError(f"trustees must be 1 .. {MAX_TRUSTEES}, not {trustees!r}")
    if not ids or len(set(ids)) != len(ids) or any(isinstance(i, bool) or not isinstance(i, int) or not 1 <= i <= trustees for i in ids):
        raise ValueError("ids must be distinct integers in 1 .. trustees")
    delta = math.factorial(trustees)
    out = []
    for i in ids:
        num, den = delta, 1
        for j in ids:
            if j != i:
                num *= j
                den *= j - i
        assert num % den == 0, "a Lagrange exponent is an integer"
        out.append(num // den)
    return out


def deal_shamir(p: int, q: int, trustees: int, threshold: int, g: Optional[int] = None,
                rand: Callable[[int], int] = secrets.randbelow) -> Tuple[ShamirKey, List[int]]:
    """The dealer of a t-of-T key: (public ShamirKey, [s_1 .. s_T]) for the key with primes p and q.  With N = n lam and theta =
    lam (lam^-1 mod n): a_1 .. a_{t-1} = rand(N) each, f(X) = theta + sum a_k X^k, s_i = f(i) mod N; v is chosen and, for safe primes,
    order-checked exactly as deal_shares does; mu2 = (2 a trustees!)^-1 mod n.  Any t - 1 shares are independent of theta.  Refuses what
    deal_shares refuses, a threshold outside 1 .. trustees, and primes that do not exceed trustees (trustees! must be a unit mod n):
    ValueError.  The dealer must forget p, q, lam, theta, the polynomial and the shares it hands out."""
    n, g, lam, _ = secret_from_primes(p, q, g)
    if isinstance(trustees, bool) or not isinstance(trustees, int) or not 1 <= trustees <= MAX_TRUSTEES:
        raise ValueError(f"trustees must be 1 .. {MAX_TRUSTEES}, not {trustees!r}")
    if isinstance(threshold, bool) or not isinstance(threshold, int) or not 1 <= threshold <= trustees:
        raise ValueError(f"threshold must be 1 .. trustees, not {threshold!r}")
    if min(p, q) <= trustees:
        raise ValueError("trustees! is not a unit mod n: the primes must exceed the number of trustees")
    n2, N = n * n, n * lam
    theta = lam * pow(lam, -1, n)
    coeffs = [theta] + [rand(N) for _ in range(threshold - 1)]
    shares = []
    for i in range(1, trustees + 1):
        s = 0
        for a in reversed(coeffs):          # Horner
            s = (s * i + a) % N
        shares.append(s)
    pp, qq = (p - 1) // 2, (q - 1) // 2
    safe = _is_prime(pp) and _is_prime(qq) and pp != qq
    half = N // 2
    while True:
        w = rand(n2)
        if w < 2 or math.gcd(w, n) != 1:
            continue
        v = w * w % n2
        if v == 1:
            continue
        if not safe or (pow(v, half, n2) == 1 and all(pow(v, half // l, n2) != 1 for l in (p, q, pp, qq))):
            break
    a = (pow(g, theta, n2) - 1) // n
    key = ShamirKey(n=n, g=g, v=v, hs=tuple(pow(v, s, n2) for s in shares), mu2=pow(2 * a * math.factorial(trustees), -1, n),
                    trustees=trustees, threshold=threshold, v_order_proved=safe)
    return key, shares


# ---------------------------------------------------------------------------------------------------------------------------------
# short randomness: the extra element hs of a Damgard-Jurik-Nielsen ("DJN mode") public key
# ---------------------------------------------------------------------------------------------------------------------------------
def djn_generator(engine, n: int, rand: Callable[[int], int] = secrets.randbelow) -> int:
    """hs = (-x^2 mod n)^n mod n^2 for a unit x drawn with rand (rand(k): uniform in [0, k), by default secrets.randbelow); the power
    is taken on the device (Engine.paillier_trace).  With it c = g^m hs^s mod n^2 for a SHORT secret s below 2^s_bits is an ordinary
    Paillier ciphertext with r = h^s mod n, h = -x^2 mod n: Engine.paillier_sballot computes it, circuit kind 'sballot' proves it, and
    tally, mix, decrypt, partial and combine take it unchanged.  Security rests on the short-exponent assumption in <hs> (the
    discrete logarithm of an element of <hs> to the base hs stays hard when it is only s_bits long): s_bits is the caller's argument
    everywhere and has no default; customary widths are at least twice the security level.  The scheme asks for p = q = 3 (mod 4), so
    that -1 is no square mod n and h generates the units of Jacobi symbol 1 up to sign: generate_key(safe=True) gives such primes.
    Nothing here shows a third party that hs is an n-th residue, i.e. an encryption of 0: the key authority shows that with circuit
    kind 'decrypt', or with kind 'partial' and a combiner."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 15 or n % 2 == 0:
        raise ValueError("n must be an odd modulus")
    while True:
        x = rand(n)
        if x >= 2 and math.gcd(x, n) == 1:
            break
    h = (-x * x) % n
    limbs = (n.bit_length() + 63) // 64
    res, _, _ = engine.paillier_trace(2 * limbs, _words(n * n, 2 * limbs), _words(h, 2 * limbs), _words(n, limbs), limbs, want_steps=False)
    return sum(int(w) << (64 * i) for i, w in enumerate(res.tolist()))


# ---------------------------------------------------------------------------------------------------------------------------------
# packed plaintexts: K choices in one ciphertext, M = sum_j v_j 2^(j w)
# ---------------------------------------------------------------------------------------------------------------------------------
def _slot_shape(slots: int, slot_bits: int) -> None:
    for x in (slots, slot_bits):
        if isinstance(x, bool) or not isinstance(x, int) or x < 1:
            raise ValueError("slots and slot_bits are positive integers")


def pack_choices(values: Sequence[int], slot_bits: int) -> int:
    """M = sum_j v_j 2^(j slot_bits): slot j of the packed plaintext holds values[j].  Every value is below 2^slot_bits."""
    _slot_shape(max(len(values), 1), slot_bits)
    if len(values) < 1 or any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < (1 << slot_bits) for v in values):
        raise ValueError("a packed plaintext has at least one slot and every value is in [0, 2^slot_bits)")
    return sum(v << (j * slot_bits) for j, v in enumerate(values))


def unpack_tally(M: int, slots: int, slot_bits: int) -> List[int]:
    """the `slots` counts of a decrypted packed total: count j is bits j slot_bits .. (j + 1) slot_bits of M.  Refuses an M of more than
    slots * slot_bits bits: no product of packed ballots within pballot_capacity decrypts to one."""
    _slot_shape(slots, slot_bits)
    if isinstance(M, bool) or not isinstance(M, int) or M < 0 or M >> (slots * slot_bits):
        raise ValueError("a packed total is in [0, 2^(slots slot_bits))")
    mask = (1 << slot_bits) - 1
    return [(M >> (j * slot_bits)) & mask for j in range(slots)]


def pballot_capacity(slot_bits: int, m_bits: int) -> int:
    """how many packed ballots whose slot values are below 2^m_bits one slot of slot_bits bits holds before it carries into the next:
    floor((2^slot_bits - 1) / (2^m_bits - 1)).  The tally of more ballots than this is not the per-slot sums."""
    _slot_shape(m_bits, slot_bits)
    if m_bits > slot_bits:
        raise ValueError("a slot value of m_bits bits does not fit a slot of slot_bits bits")
    return ((1 << slot_bits) - 1) // ((1 << m_bits) - 1)


def pballot_bases(engine, n: int, g: int, slots: int, slot_bits: int) -> List[int]:
    """the public slot bases G_j = g^(2^(j slot_bits)) mod n^2, j = 0 .. slots - 1, of a packed ballot (Engine.paillier_pballot): read
    from the squaring records of ONE Engine.paillier_trace of g^(2^((slots - 1) slot_bits)) -- bit t of that exponent below its top
    one is clear, so record t is the square whose remainder is g^(2^(t + 1)), and the remainder of record j slot_bits - 1 is G_j.
    Refuses 2^(slots slot_bits) > n: the packed plaintext must stay below n."""
    _slot_shape(slots, slot_bits)
    if isinstance(n, bool) or not isinstance(n, int) or n < 15 or n % 2 == 0:
        raise ValueError("n must be an odd modulus")
    if (1 << (slots * slot_bits)) > n:
        raise ValueError("the packed plaintext of slots * slot_bits bits must stay below n")
    if not 0 < int(g) < n * n:
        raise ValueError("g is in [1, n^2)")
    top = (slots - 1) * slot_bits
    if top == 0:
        return [int(g)]
    limbs = (n.bit_length() + 63) // 64
    e_limbs = top // 64 + 1
    _, steps, ns = engine.paillier_trace(2 * limbs, _words(n * n, 2 * limbs), _words(int(g), 2 * limbs), _words(1 << top, e_limbs), e_limbs)
    if ns != top + 2:
        raise RuntimeError("the trace of a power of two has one record per bit and one product")
    word = lambda row: sum(int(w) << (64 * i) for i, w in enumerate(row.tolist()))
    return [int(g)] + [word(steps[j * slot_bits - 1, 3]) for j in range(1, slots)]


# ---------------------------------------------------------------------------------------------------------------------------------
# prime generation: the search runs on the device -- an engine is required, there is no CPU fallback
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_PRIME_BITS = 2048        # 32 words: what pz_bigint_is_prime / pz_prime_search take
MIN_PRIME_BITS = 40          # a window's start must exceed 2^32, with room for the window below 2^bits
MAX_WINDOW = 1 << 20


def _words(x: int, limbs: int) -> List[int]:
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(limbs)]


def _bases(rounds: int, rand: Callable[[int], int]) -> List[int]:
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= 64:
        raise ValueError(f"rounds must be 1 .. 64, not {rounds!r}")
    return [rand(64) | 2 for _ in range(rounds)]


def is_probable_prime(engine, xs, rounds: int = 32, rand: Callable[[int], int] = secrets.randbits) -> List[bool]:
    """Miller-Rabin on the device for every integer of xs (0 <= x < 2^2048) over `rounds` bases rand(64) | 2 drawn for this call
    (rand(k): k random bits, by default secrets.randbits): True where x passes every round.  One Engine.is_prime call."""
    xs = list(xs)
    if not xs or any(isinstance(x, bool) or not isinstance(x, int) or x < 0 or x.bit_length() > MAX_PRIME_BITS for x in xs):
        raise ValueError(f"xs: a non-empty list of integers in [0, 2^{MAX_PRIME_BITS})")
    limbs = max(1, max((x.bit_length() + 63) // 64 for x in xs))
    flags, _ = engine.is_prime(limbs, [_words(x, limbs) for x in xs], _bases(rounds, rand))
    return [bool(f) for f in flags]


def default_window(bits: int, safe: bool) -> int:
    """offsets one search covers: about eight expected gaps between primes of `bits` bits at stride 2 (a gap is ~0.35 bits offsets),
    about two and a half expected gaps between safe primes at stride 4 (~0.05 bits^2 offsets), as powers of two within 2^10 .. 2^20"""
    want = bits * bits // 8 if safe else 4 * bits
    return min(MAX_WINDOW, max(1 << 10, 1 << (want - 1).bit_length()))


def generate_prime(engine, bits: int, safe: bool = False, rounds: int = 32, rand: Callable[[int], int] = secrets.randbits,
                   window: Optional[int] = None) -> int:
    """A probable prime of exactly `bits` bits with its two top bits set (so that the product of two has exactly the sum of their
    bits), found on the device; with safe, (p - 1) / 2 is a probable prime too.  Per window a fresh start rand(bits) with the top two
    bits and the residue forced (odd; 3 mod 4 with safe) and fresh bases; Engine.prime_search returns the smallest offset that
    survives the sieve and every round, and the loop draws again until a window yields one.  window defaults to default_window."""
    if isinstance(bits, bool) or not isinstance(bits, int) or not MIN_PRIME_BITS <= bits <= MAX_PRIME_BITS:
        raise ValueError(f"bits must be {MIN_PRIME_BITS} .. {MAX_PRIME_BITS}, not {bits!r}")
    stride, residue = (4, 3) if safe else (2, 1)
    if window is None:
        window = default_window(bits, safe)
    if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= MAX_WINDOW:
        raise ValueError(f"window must be 1 .. {MAX_WINDOW}, not {window!r}")
    limbs = (bits + 63) // 64
    while True:
        start = (rand(bits) & ((1 << bits) - 1)) | (3 << (bits - 2))
        start = start - start % stride + residue
        if start + stride * (window - 1) >> bits:
            continue                                        # the window would leave the bit length: draw again
        offsets, _ = engine.prime_search(limbs, _words(start, limbs), window, safe, _bases(rounds, rand), 1)
        if len(offsets):
            return start + stride * int(offsets[0])


def generate_key(engine, bits: int, safe: bool = False, rounds: int = 32, rand: Callable[[int], int] = secrets.randbits,
                 window: Optional[int] = None) -> Tuple[int, int]:
    """(p, q) for secret_from_primes, deal_shares and deal_shamir: probable primes of bits // 2 and bits - bits // 2 bits from
    generate_prime with p != q, n = p q of exactly `bits` bits and gcd(n, phi(n)) = 1; with safe both are safe primes and
    (p - 1) / 2 != (q - 1) / 2, which is what gives the dealers' keys v_order_proved = True."""
    if isinstance(bits, bool) or not isinstance(bits, int) or bits < 2 * MIN_PRIME_BITS:
        raise ValueError(f"bits must be {2 * MIN_PRIME_BITS} .. {2 * MAX_PRIME_BITS}, not {bits!r}")
    while True:
        p = generate_prime(engine, bits // 2, safe, rounds, rand, window)
        q = generate_prime(engine, bits - bits // 2, safe, rounds, rand, window)
        n = p * q
        if p != q and n.bit_length() == bits and math.gcd(n, (p - 1) * (q - 1)) == 1:
            return p, q
