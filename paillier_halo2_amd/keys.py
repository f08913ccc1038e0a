"""Paillier secret keys as Python integers: what Engine.paillier_sk (pz.h pz_paillier_sk_create) takes.

The library derives mu and g^-1 on the device and validates the key there; the one value it does not derive is d = n^-1 mod lambda,
the exponent that recovers an encryption's randomness: it is the caller's, and this helper computes it."""
from __future__ import annotations

import math
from typing import Optional, Tuple


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
