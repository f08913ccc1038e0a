"""Test helper (not product code): the 64-byte G2 format of DESIGN.md section 15.4 in Python integers, on tests/bn254_pairing_ref.py's
Fq2 and twist.  Its own square root (the complex method over pow(., (p+1)/4)), its own codec, and the twist points outside the order-r
subgroup that pz_g2_check must tell apart.

G2 point, 64 bytes: canonical x.c0 little-endian | canonical x.c1 little-endian, bit 7 of byte 63 = y.c0 & 1, bit 6 of byte 63 zero, the
identity 64 zero bytes.  y.c0 = 0: the bit is 0 and the decoder returns the root with an even y.c1 (include/pz.h)."""
import random

from tests import bn254_pairing_ref as B

P, R = B.P, B.R
OK, NOT_CANONICAL, OFF_TWIST, NOT_IN_SUBGROUP = 0, 1, 2, 3
COFACTOR = 2 * P - R          # #E'(Fq2) = r (2p - r) for a BN curve's sextic twist
assert P % 4 == 3 and COFACTOR % 10069 == 0 and COFACTOR % 5864401 == 0


def fq_sqrt(a):
    """-> a square root of a in Fq, or None"""
    c = pow(a, (P + 1) // 4, P)
    return c if c * c % P == a % P else None


def f2_sqrt(a):
    """-> a square root of a = (a0, a1) in Fq2 = Fq[u]/(u^2 + 1), or None.  a1 = 0: (sqrt(a0), 0), else (0, sqrt(-a0)) (-1 is not a square).
    Otherwise N = a0^2 + a1^2 must be a square s^2; t = (a0 + s)/2 or (a0 - s)/2 is x0^2, x1 = a1 / (2 x0)."""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        c = fq_sqrt(a0)
        if c is not None:
            return (c, 0)
        c = fq_sqrt(-a0 % P)
        return None if c is None else (0, c)
    s = fq_sqrt((a0 * a0 + a1 * a1) % P)
    if s is None:
        return None
    half = (P + 1) // 2
    x0 = fq_sqrt((a0 + s) * half % P)
    if x0 is None:
        x0 = fq_sqrt((a0 - s) * half % P)
        if x0 is None:
            return None
    return (x0, a1 * pow(2 * x0, -1, P) % P)


def rhs(x):
    return B.f2_add(B.f2_mul(B.f2_sqr(x), x), B.B2)


def compress(q) -> bytes:
    """q: ((x0, x1), (y0, y1)) canonical integers on the twist, or None for the identity"""
    if q is None:
        return bytes(64)
    (x0, x1), (y0, _) = q
    assert B.g2_on_curve(q) and max(x0, x1) < P
    return x0.to_bytes(32, "little") + (x1 | (y0 & 1) << 255).to_bytes(32, "little")


def decompress(b: bytes):
    """-> (status, point): point is None for the identity and for a refused encoding"""
    assert len(b) == 64
    x0 = int.from_bytes(b[:32], "little")
    v = int.from_bytes(b[32:], "little")
    sign, x1 = v >> 255, v & ((1 << 255) - 1)
    if x0 >= P or x1 >= P:
        return NOT_CANONICAL, None
    if x0 == 0 and x1 == 0 and sign == 0:
        return OK, None
    w = rhs((x0, x1))
    y = f2_sqrt(w)
    if y is None or B.f2_sqr(y) != w:
        return OFF_TWIST, None
    flip = (y[1] & 1) != 0 if y[0] == 0 else (y[0] & 1) != sign
    return OK, ((x0, x1), B.f2_neg(y) if flip else y)


def check(q) -> int:
    """pz_g2_check's status of a point given as canonical integers (None = the identity)"""
    if q is None:
        return OK
    if max(q[0] + q[1]) >= P:
        return NOT_CANONICAL
    if not B.g2_on_curve(q):
        return OFF_TWIST
    return OK if B.g2_mul(q, R, reduce=False) is None else NOT_IN_SUBGROUP


def random_twist_point(rng: random.Random):
    """a uniformly drawn x with a root: a point of the twist, in the order-r subgroup only with probability 1 / cofactor"""
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = f2_sqrt(rhs(x))
        if y is not None:
            return (x, y)


def x_without_root(rng: random.Random):
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        if f2_sqrt(rhs(x)) is None:
            return x


def point_of_order_10069(rng: random.Random):
    """[r (2p - r) / 10069] T for random T until it is not the identity: its order divides the prime 10069"""
    while True:
        q = B.g2_mul(random_twist_point(rng), R * (COFACTOR // 10069), reduce=False)
        if q is not None:
            return q
