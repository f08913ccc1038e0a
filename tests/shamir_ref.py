"""Test-side restatement of t-of-T threshold decryption with Shamir shares, independent of the product and in
Python integers alone: the modular inverse (pow(x, -1, m)), the dealing (a polynomial of degree t - 1 over Z_(n lambda) with f(0) =
theta = lambda (lambda^-1 mod n)), the Lagrange exponents (as fractions, their integrality checked) and the combination by the sign
split: A over the positive exponents, B over the negative ones, A = B (1 + x n) mod n^2.  The product must not import this module."""
import math
from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

# two 64-bit safe primes (p and (p - 1) / 2 both prime, found once with paillier_halo2_amd.keys._is_prime): a 128-bit n
SAFE_P, SAFE_Q = 0xA4E4E25A2BF9133F, 0xF6CC057211D86F37

F_MISMATCH, F_RANGE, F_INTERNAL, F_NOT_UNIT = 1, 2, 4, 8       # the combiner's flag bits
INV_NOT_UNIT, INV_RANGE = 1, 2                                # the inverse's


def inverse(x: int, m: int) -> Tuple[int, int]:
    """-> (x^-1 mod m, flags) as pz_bigint_mod_inverse reports an entry: zero with bit 1 where x >= m, zero with bit 0 where x is no unit"""
    if x >= m:
        return 0, INV_RANGE
    if math.gcd(x, m) != 1:
        return 0, INV_NOT_UNIT
    return pow(x, -1, m), 0


def lam_of(p: int, q: int) -> int:
    return (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)


def theta_of(p: int, q: int) -> int:
    lam = lam_of(p, q)
    return lam * pow(lam, -1, p * q)


def pow_n2(b: int, e: int, p: int, q: int) -> int:
    """b^e mod n^2 for a unit b, by the Chinese remainder theorem over p^2 and q^2 (the tests know the primes): pow(b, e, n * n), three
    times quicker, which is what keeps the 2048- and 3072-bit cases short.  tests/test_shamir.py holds it to pow() itself."""
    p2, q2 = p * p, q * q
    if b % p == 0 or b % q == 0:
        return pow(b, e, p2 * q2)
    xp, xq = pow(b % p2, e % (p * (p - 1)), p2), pow(b % q2, e % (q * (q - 1)), q2)
    return xp + p2 * ((xq - xp) * pow(p2, -1, q2) % q2)


def deal(p: int, q: int, trustees: int, threshold: int, rand, g: Optional[int] = None):
    """-> (n, g, [s_1 .. s_T], mu2): a_1 .. a_{t-1} = rand(N) each, s_i = theta + sum_k a_k i^k mod N, mu2 = (2 a T!)^-1 mod n"""
    n = p * q
    N = n * lam_of(p, q)
    g = n + 1 if g is None else g
    theta = theta_of(p, q)
    coeffs = [theta] + [rand(N) for _ in range(threshold - 1)]
    shares = [sum(a * i ** k for k, a in enumerate(coeffs)) % N for i in range(1, trustees + 1)]
    a = (pow_n2(g, theta, p, q) - 1) // n
    return n, g, shares, pow(2 * a * math.factorial(trustees), -1, n)


def lagrange(trustees: int, ids: Sequence[int]) -> List[int]:
    """mu_i = T! prod_{j in ids, j != i} j / (j - i) as exact fractions; every one must be an integer"""
    out = []
    for i in ids:
        mu = Fraction(math.factorial(trustees))
        for j in ids:
            if j != i:
                mu *= Fraction(j, j - i)
        assert mu.denominator == 1, (trustees, list(ids), i)
        out.append(int(mu))
    return out


def partial(c: int, share: int, n: int, pq: Optional[Tuple[int, int]] = None) -> int:
    """u = (c^2)^share mod n^2 (pq = the primes: the same through pow_n2)"""
    return pow(c * c % (n * n), share, n * n) if pq is None else pow_n2(c * c % (n * n), share, *pq)


def split_products(mus: Sequence[int], us: Sequence[int], n: int) -> Tuple[int, int]:
    """(A, B) = (prod_{mu > 0} u^mu, prod_{mu < 0} u^|mu|) mod n^2"""
    n2 = n * n
    A = B = 1
    for mu, u in zip(mus, us):
        if mu > 0:
            A = A * pow(u, mu, n2) % n2
        else:
            B = B * pow(u, -mu, n2) % n2
    return A, B


def combine(mus: Sequence[int], us: Sequence[int], n: int, mu2: int) -> Tuple[int, int]:
    """-> (m, flags) as pz_paillier_combine_t reports one ciphertext"""
    n2 = n * n
    if any(u >= n2 for u in us):
        return 0, F_RANGE
    A, B = split_products(mus, us, n)
    flags = 0
    if A % n != B % n:
        flags |= F_MISMATCH
    if math.gcd(B % n, n) != 1:
        flags |= F_NOT_UNIT
    if flags:
        return 0, flags
    x = (A - B) % n2 // n * pow(B % n, -1, n) % n
    return x * mu2 % n, 0


def encrypt(n: int, g: int, m: int, r: int, pq: Optional[Tuple[int, int]] = None) -> int:
    if pq is None:
        return pow(g, m, n * n) * pow(r, n, n * n) % (n * n)
    return pow_n2(g, m, *pq) * pow_n2(r, n, *pq) % (n * n)
