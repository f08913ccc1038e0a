"""Structured operands for the curve stack -- Fq in 29-bit limbs, G1 in XYZZ, the MSM, Fq2 .. Fq12, G2 and the pairing (csrc/fp29.cuh,
ec29.cuh, ec29_quad.cuh, pz_msm.hip, fp12.cuh, pz_pairing.hip) -- and a model of the MSM's signed-digit recoding in Python integers
(DESIGN.md section 15.14).  The catalogue: G1 points with tiny and near-p coordinates and [k]G at the ends of the scalar range, each
also as Jacobian triples under several Z; scalars at every window boundary of the window widths the tests load, the
all-windows-equal digit patterns and their negations; G2 multiples; one twist point outside the r-subgroup.  `recode` restates
scalar_prepare + next_digit.  Pure Python, its own moduli and its own point arithmetic; the product must not import this module."""
import functools
import random
from typing import Dict, List, Optional, Tuple

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = 1 << 256
HALF = (R - 1) // 2
assert P % 4 == 3 and P % 3 == 1            # the (p+1)/4 square root; cube roots need the 3-Sylow subgroup (cbrt_fq)

Affine = Tuple[int, int]
INF: Affine = (0, 0)            # halo2curves' affine identity; no point has x = 0 because 3 is a non-residue (test_curve_operands.py)
G: Affine = (1, 2)

WINDOWS = (4, 5, 8, 11, 13, 15, 16)      # the window widths the scalar catalogue aims at
LAMBDAS = (1, 2, P - 1, 0x1D0C7A1B5E3F60927384A5B6C7D8E9F00112233445566778899AABBCCDDEEFF1 % P)


# ---- the curve in plain affine integers ------------------------------------------------------------------------------------------------
def on_curve(pt: Affine) -> bool:
    return pt == INF or (0 <= pt[0] < P and 0 <= pt[1] < P and (pt[1] * pt[1] - pt[0] ** 3 - 3) % P == 0)


def neg(pt: Affine) -> Affine:
    return pt if pt == INF else (pt[0], (P - pt[1]) % P)


def add(a: Affine, b: Affine) -> Affine:
    if a == INF:
        return b
    if b == INF:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return INF
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return (x3, (lam * (x1 - x3) - y1) % P)


def mul(pt: Affine, k: int) -> Affine:
    """[k] pt for any integer k >= 0 (NOT reduced mod r: the order of a structured point is what a test asserts)"""
    acc = INF
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def sqrt_fq(a: int) -> Optional[int]:
    y = pow(a % P, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def _cbrt_setup():
    s, t = 0, P - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    g = 2
    while pow(g, (P - 1) // 3, P) == 1:
        g += 1
    return s, t, pow(g, t, P)           # a generator of the 3-Sylow subgroup (order 3^s)


_CB_S, _CB_T, _CB_G = _cbrt_setup()


def cbrt_fq(a: int) -> Optional[int]:
    """one cube root of a mod p, None if there is none (p = 1 mod 3: a third of Fq* are cubes)"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 3, P) != 1:
        return None
    # a = u * h with h in the 3-Sylow subgroup: u^(1/3) by inverting 3 mod t, h^(1/3) by a search over the subgroup (3^s elements, s small)
    e = pow(3, -1, _CB_T)
    x = pow(a, e, P)                    # x^3 = a * a^(3e - 1), and a^(3e-1) has order dividing 3^s
    h = a * pow(x, -3, P) % P
    z = 1
    for _ in range(3 ** _CB_S):
        if pow(z, 3, P) == h:
            x = x * z % P
            assert pow(x, 3, P) == a
            return x
        z = z * _CB_G % P
    raise AssertionError("no cube root of a cubic residue")


# ---- G1 points ---------------------------------------------------------------------------------------------------------------------------
K_CONST = (1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2)
K_NAMES = ("1", "2", "3", "r-1", "r-2", "(r-1)/2", "(r+1)/2")


def _first(n: int, gen):
    out = []
    for v in gen:
        if v is not None:
            out.append(v)
            if len(out) == n:
                return out
    raise AssertionError


def _by_x(xs):
    for x in xs:
        y = sqrt_fq(x ** 3 + 3)
        yield None if y is None else (x % P, min(y, P - y))


def _by_y(ys):
    for y in ys:
        x = cbrt_fq(y * y - 3)
        yield None if x is None else (x, y)


@functools.lru_cache(maxsize=None)
def g1_roots() -> Tuple[Tuple[str, Affine], ...]:
    """the named structured points before negation: [k]G, the four smallest x, the four largest x, the four smallest y.  Of the two
    roots of x^3 + 3 the smaller one is listed (its negation, with y near p or above p/2, is in g1_points)"""
    out = [("[%s]G" % nm, mul(G, k)) for nm, k in zip(K_NAMES, K_CONST)]
    out += [("x=%d" % pt[0], pt) for pt in _first(4, _by_x(range(1, 1000)))]
    out += [("x=p-%d" % (P - pt[0]), pt) for pt in _first(4, _by_x(range(P - 1, P - 1000, -1)))]
    out += [("y=%d" % pt[1], pt) for pt in _first(4, _by_y(range(1, 1000)))]
    for _, pt in out:
        assert on_curve(pt) and pt != INF
    return tuple(out)


@functools.lru_cache(maxsize=None)
def g1_points() -> Tuple[Tuple[str, Affine], ...]:
    """every structured point, its negation and the identity; a point that appears twice (G is [1]G, x = 1 and y = 2; [r-1]G is -G)
    keeps its first name"""
    seen: Dict[Affine, str] = {}
    for nm, pt in g1_roots():
        seen.setdefault(pt, nm)
    for nm, pt in g1_roots():
        seen.setdefault(neg(pt), "-" + nm)
    seen.setdefault(INF, "identity")
    return tuple((nm, pt) for pt, nm in seen.items())


@functools.lru_cache(maxsize=None)
def g1_pairing_points() -> Tuple[Tuple[str, Affine], ...]:
    """the list the word-for-word pairing test runs (the reference pairing takes ~0.15 s): the distinct structured roots, the identity,
    and the negations of the roots x = 2 and x = p - 1 (y near p) -- 20 points, 40 pairings with two G2 arguments; the other negations
    reach the pairing through pairing_check, where the expected value is an integer identity and costs nothing"""
    seen: Dict[Affine, str] = {}
    for nm, pt in g1_roots():
        seen.setdefault(pt, nm)
    seen.setdefault(INF, "identity")
    roots = dict(g1_roots())
    for nm in ("x=2", "x=p-1"):
        seen.setdefault(neg(roots[nm]), "-" + nm)
    assert len(seen) == 20
    return tuple((nm, pt) for pt, nm in seen.items())


def jacobian(pt: Affine, lam: int) -> Tuple[int, int, int]:
    """(lam^2 x, lam^3 y, lam); the identity keeps non-zero X and Y over Z = 0"""
    lam %= P
    assert lam
    if pt == INF:
        return (lam * lam % P, lam ** 3 % P, 0)
    return (lam * lam * pt[0] % P, lam ** 3 * pt[1] % P, lam)


def fq_words(x: int) -> List[int]:
    m = (x % P) * MONT % P
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def fq_from_words(ws) -> int:
    return sum(int(w) << (64 * i) for i, w in enumerate(ws)) * pow(MONT, -1, P) % P


def fr_words(s: int) -> List[int]:
    m = (s % R) * MONT % R
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def aff_words(pt: Affine) -> List[int]:
    return fq_words(pt[0]) + fq_words(pt[1])


def aff_from_words(ws) -> Affine:
    return (fq_from_words(ws[0:4]), fq_from_words(ws[4:8]))


def jac_words(pt: Affine, lam: int) -> List[int]:
    X, Y, Z = jacobian(pt, lam)
    return fq_words(X) + fq_words(Y) + fq_words(Z)


# ---- scalars -----------------------------------------------------------------------------------------------------------------------------
def n_windows(c: int) -> int:
    return 253 // c + 1


SCALAR_CONSTANTS = (0, 1, 2, R - 1, R - 2, HALF, HALF + 1, HALF - 1, HALF + 2)     # (r+1)/2 is (r-1)/2 + 1; (r+1)/2 + 1 added


def boundary_scalars(c: int) -> List[int]:
    """2^k and 2^k +- 1 for k in {cw - 1, cw, cw + 1}, every window w of width c, below r"""
    out = []
    for w in range(n_windows(c)):
        for k in (c * w - 1, c * w, c * w + 1):
            if k >= 0:
                out += [v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= v < R]
    return out


def pattern_digits(c: int) -> Tuple[int, ...]:
    return (1, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1)


def pattern_scalar(c: int, d: int) -> int:
    """every window's raw digit equal to d, the top windows lowered (to the largest digit that fits, zero if none) until the value is
    at most (r - 1)/2 -- so the device recodes the value itself, not its negation"""
    assert 0 < d < (1 << c)
    digs = [d] * n_windows(c)
    val = lambda: sum(x << (c * w) for w, x in enumerate(digs))
    for w in reversed(range(len(digs))):
        if val() <= HALF:
            break
        digs[w] = 0
        room = (HALF - val()) >> (c * w)
        digs[w] = max(0, min(d, room))
    v = val()
    assert 0 < v <= HALF
    return v


@functools.lru_cache(maxsize=None)
def scalars_for(c: int) -> Tuple[int, ...]:
    """the catalogue at one window width: constants, that width's boundaries and patterns, and r - s of each"""
    base = list(SCALAR_CONSTANTS) + boundary_scalars(c) + [pattern_scalar(c, d) for d in pattern_digits(c)]
    seen: Dict[int, None] = {}
    for s in base:
        seen.setdefault(s % R)
    for s in base:
        seen.setdefault((R - s) % R)
    return tuple(seen)


@functools.lru_cache(maxsize=None)
def scalars_all() -> Tuple[int, ...]:
    seen: Dict[int, None] = {}
    for c in WINDOWS:
        for s in scalars_for(c):
            seen.setdefault(s)
    return tuple(seen)


def recode(s: int, c: int, fold: bool = True) -> Tuple[bool, List[int], int]:
    """scalar_prepare + next_digit of pz_msm.hip: (neg, digits, carry out of the last window) for the canonical scalar s in [0, r).
    neg = (r - s < s); the digits are those of min(s, r - s), one per window 0 .. 253/c, each in (-2^(c-1), 2^(c-1)].
    fold = False recodes s itself (what a sign fold that is not taken would leave)"""
    assert 0 <= s < R and 4 <= c <= 16
    t = R - s
    negate = fold and t < s
    m = t if negate else s
    digits, carry = [], 0
    for w in range(n_windows(c)):
        raw = (m >> (c * w)) & ((1 << c) - 1)
        d = raw + carry
        if d > (1 << (c - 1)):
            carry = 1
            d -= 1 << c
        else:
            carry = 0
        digits.append(d)
    return negate, digits, carry


BRANCHES = ("carry_in_to_zero", "half_no_carry", "half_plus_one", "carry_through_all", "fold_taken", "fold_not_taken")


def branches(s: int, c: int) -> Tuple[str, ...]:
    """which of the recoding's branches the scalar s takes at width c"""
    t = R - s
    negate = t < s
    m = t if negate else s
    hit = {"fold_taken" if negate else "fold_not_taken"}
    carry, carries = 0, []
    for w in range(n_windows(c)):
        raw = (m >> (c * w)) & ((1 << c) - 1)
        d = raw + carry
        if carry and raw == (1 << c) - 1:
            hit.add("carry_in_to_zero")
        if not carry and d == 1 << (c - 1):
            hit.add("half_no_carry")
        if d == (1 << (c - 1)) + 1:
            hit.add("half_plus_one")
        carry = 1 if d > (1 << (c - 1)) else 0
        carries.append(carry)
    # a carry out of every window below the last one that holds a bit of m (the last window's own digit then absorbs it)
    top = (m.bit_length() - 1) // c if m else 0
    if top >= n_windows(c) - 2 and all(carries[:top]):
        hit.add("carry_through_all")
    return tuple(b for b in BRANCHES if b in hit)


def branch_table(c: int) -> Dict[str, int]:
    out = {b: 0 for b in BRANCHES}
    for s in scalars_for(c):
        for b in branches(s, c):
            out[b] += 1
    return out


# ---- G2 ----------------------------------------------------------------------------------------------------------------------------------
def g2_points():
    """[(name, point)]: [k]G2 for the constant k, the negations, the identity (None), in tests/bn254_pairing_ref.py's representation"""
    from tests import bn254_pairing_ref as B

    seen = {}
    for nm, k in zip(K_NAMES, K_CONST):
        seen.setdefault(B.g2_mul(B.G2, k), "[%s]G2" % nm)
    for q, nm in list(seen.items()):
        seen.setdefault(B.g2_neg(q), "-" + nm)
    out = [(nm, q) for q, nm in seen.items()]
    out.append(("identity", None))
    return out


def twist_point_outside_subgroup():
    """a point of the twist E'(Fq2) that is not in the r-subgroup, built as tests/test_gpu_params.py builds it; for g2_check only,
    never a pairing argument"""
    from tests import g2_wire_ref as G2W

    return G2W.random_twist_point(random.Random(1))
