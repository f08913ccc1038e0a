"""Paillier secret keys as Python integers: what Engine.paillier_sk (pz.h pz_paillier_sk_create) takes, and the dealer of a T-of-T
threshold key (deal_shares): additive shares of the decryption exponent for Engine.paillier_partial and the
public ThresholdKey for Engine.paillier_combine and the verifier of circuit kind 'partial'.

The library derives mu and g^-1 on the device and validates the key there; the one value it does not derive is d = n^-1 mod lambda,
the exponent that recovers an encryption's randomness: it is the caller's, and this helper computes it."""
from __future__ import annotations

import math
import secrets
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple


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
    """Miller-Rabin over the first twelve primes (deterministic below 3.3e24) and 24 more fixed bases above"""
    if x < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for s in small:
        if x % s == 0:
            return x == s
    d, r = x - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    bases = small if x < 3317044064679887385961981 else small + tuple(range(41, 137, 4))
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
