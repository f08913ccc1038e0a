"""Python restatement of the BN254 optimal-ate pairing (Python ints), the yardstick of the HIP pairing in csrc/pz_pairing.hip.

halo2curves' tower: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi) with xi = 9 + u, Fq12 = Fq6[w]/(w^2 - v).  G2 is the
D-type twist y^2 = x^3 + 3/xi over Fq2, untwisted by (x, y) -> (x w^2, y w^3).  The Miller loop here is affine and binary
(the kernel's is projective, with lines scaled by Fq2 factors): the two agree only after the final exponentiation, which
is plain exponentiation by (p^12 - 1)/r, so a match is a real check of both.

Elements: Fq2 = (c0, c1); Fq6 = (a0, a1, a2) of Fq2; Fq12 = (b0, b1) of Fq6.  Integers are canonical, not Montgomery.
"""
from __future__ import annotations

X = 0x44E992B44A6909F1
P = 36 * X**4 + 36 * X**3 + 24 * X**2 + 6 * X + 1
R = 36 * X**4 + 36 * X**3 + 18 * X**2 + 6 * X + 1
ATE = 6 * X + 2
MONT = 1 << 256
HARD = (P**4 - P**2 + 1) // R
FINAL = (P**12 - 1) // R

G1 = (1, 2)
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
       11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930,
       4082367875863433681332203403145435568316851327593401208105741076214120093531))


# ---------------------------------------------------------------- Fq2
def f2(a, b=0):
    return (a % P, b % P)


F2_ZERO, F2_ONE = (0, 0), (1, 0)
XI = (9, 1)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return ((-a[0]) % P, (-a[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_muls(a, s):
    return (a[0] * s % P, a[1] * s % P)


def f2_sqr(a):
    return f2_mul(a, a)


def f2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * d % P, (-a[1]) * d % P)


def f2_conj(a):
    return (a[0], (-a[1]) % P)


def f2_pow(a, e):
    r = F2_ONE
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_sqr(a)
        e >>= 1
    return r


def f2_mul_xi(a):
    return f2_mul(a, XI)


# ---------------------------------------------------------------- Fq6
F6_ZERO = (F2_ZERO, F2_ZERO, F2_ZERO)
F6_ONE = (F2_ONE, F2_ZERO, F2_ZERO)


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(f2_neg(x) for x in a)


def f6_mul(a, b):
    # schoolbook, v^3 = xi
    c = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] = f2_add(c[i + j], f2_mul(a[i], b[j]))
    return (f2_add(c[0], f2_mul_xi(c[3])), f2_add(c[1], f2_mul_xi(c[4])), c[2])


def f6_mul_v(a):
    return (f2_mul_xi(a[2]), a[0], a[1])


def f6_inv(a):
    a0, a1, a2 = a
    t0 = f2_sub(f2_sqr(a0), f2_mul_xi(f2_mul(a1, a2)))
    t1 = f2_sub(f2_mul_xi(f2_sqr(a2)), f2_mul(a0, a1))
    t2 = f2_sub(f2_sqr(a1), f2_mul(a0, a2))
    den = f2_add(f2_mul(a0, t0), f2_mul_xi(f2_add(f2_mul(a2, t1), f2_mul(a1, t2))))
    di = f2_inv(den)
    return (f2_mul(t0, di), f2_mul(t1, di), f2_mul(t2, di))


# ---------------------------------------------------------------- Fq12
F12_ONE = (F6_ONE, F6_ZERO)


def f12_mul(a, b):
    t0 = f6_mul(a[0], b[0])
    t1 = f6_mul(a[1], b[1])
    c1 = f6_add(f6_mul(a[0], b[1]), f6_mul(a[1], b[0]))
    return (f6_add(t0, f6_mul_v(t1)), c1)


def f12_sqr(a):
    return f12_mul(a, a)


def f12_conj(a):
    return (a[0], f6_neg(a[1]))


def f12_inv(a):
    d = f6_inv(f6_sub(f6_mul(a[0], a[0]), f6_mul_v(f6_mul(a[1], a[1]))))
    return (f6_mul(a[0], d), f6_neg(f6_mul(a[1], d)))


def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_sqr(r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_is_one(a):
    return a == F12_ONE


def f12_coeffs(a):
    """the six Fq2 coefficients in the ABI order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (coefficient of w^(i + 2j) at c_i.c_j)"""
    return [a[0][0], a[0][1], a[0][2], a[1][0], a[1][1], a[1][2]]


def f12_from_coeffs(c):
    return ((c[0], c[1], c[2]), (c[3], c[4], c[5]))


W_EXP = [0, 2, 4, 1, 3, 5]   # power of w carried by the i-th ABI coefficient


def frob_consts(k):
    """gamma_{k,e} = xi^(e (p^k - 1) / 6), e = 0..5: (c w^e)^(p^k) = frob_k(c) gamma_{k,e} w^e"""
    return [f2_pow(XI, e * (P**k - 1) // 6) for e in range(6)]


def f12_frob(a, k):
    g = frob_consts(k)
    out = []
    for i, c in enumerate(f12_coeffs(a)):
        cc = f2_conj(c) if k & 1 else c
        out.append(f2_mul(cc, g[W_EXP[i]]))
    return f12_from_coeffs(out)


# ---------------------------------------------------------------- curves (affine, None = identity)
B2 = f2_mul((3, 0), f2_inv(XI))   # 3 / xi, the twist's b


def g1_on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 3) % P == 0


def g1_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], P - 2, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], P - 2, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def g1_neg(a):
    return None if a is None else (a[0], (-a[1]) % P)


def g1_mul(a, s):
    r = None
    for bit in bin(s % R)[2:] if s % R else "":
        r = g1_add(r, r)
        if bit == "1":
            r = g1_add(r, a)
    return r


def g2_on_curve(q):
    if q is None:
        return True
    x, y = q
    return f2_sub(f2_sqr(y), f2_add(f2_mul(f2_sqr(x), x), B2)) == F2_ZERO


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if f2_add(a[1], b[1]) == F2_ZERO:
            return None
        lam = f2_mul(f2_muls(f2_sqr(a[0]), 3), f2_inv(f2_muls(a[1], 2)))
    else:
        lam = f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))
    x = f2_sub(f2_sub(f2_sqr(lam), a[0]), b[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(a[0], x)), a[1]))


def g2_neg(a):
    return None if a is None else (a[0], f2_neg(a[1]))


def g2_mul(a, s, reduce=True):
    s = s % R if reduce else s
    r = None
    for bit in bin(s)[2:] if s else "":
        r = g2_add(r, r)
        if bit == "1":
            r = g2_add(r, a)
    return r


def g2_frob(q):
    """pi(Q) on the twist: (conj(x) gamma_{1,2}, conj(y) gamma_{1,3})"""
    g = frob_consts(1)
    return (f2_mul(f2_conj(q[0]), g[2]), f2_mul(f2_conj(q[1]), g[3]))


# ---------------------------------------------------------------- pairing
def _line(t, q, pt):
    """l_{T,Q}(P) in Fq12 for affine T, Q on the twist and P = (xp, yp) in G1; T = -Q gives the vertical line"""
    xp, yp = pt
    if t[0] == q[0] and f2_add(t[1], q[1]) == F2_ZERO:
        # x_P - x_T w^2: w^2 = v, the coefficient c0.c1
        return ((f2(xp), f2_neg(t[0]), F2_ZERO), F6_ZERO)
    if t == q:
        lam = f2_mul(f2_muls(f2_sqr(t[0]), 3), f2_inv(f2_muls(t[1], 2)))
    else:
        lam = f2_mul(f2_sub(q[1], t[1]), f2_inv(f2_sub(q[0], t[0])))
    # y_P - lam x_P w + (lam x_T - y_T) w^3: w -> c1.c0, w^3 -> c1.c1
    return ((f2(yp), F2_ZERO, F2_ZERO), (f2_neg(f2_muls(lam, xp)), f2_sub(f2_mul(lam, t[0]), t[1]), F2_ZERO))


def miller_loop(pairs):
    """prod_i f_{6x+2,Q_i}(P_i) l_{[6x+2]Q_i, pi(Q_i)}(P_i) l_{.., -pi^2(Q_i)}(P_i); pairs with an identity contribute 1"""
    pairs = [(pt, q) for pt, q in pairs if pt is not None and q is not None]
    f = F12_ONE
    ts = [q for _, q in pairs]
    for bit in bin(ATE)[3:]:
        f = f12_sqr(f)
        for i, (pt, q) in enumerate(pairs):
            f = f12_mul(f, _line(ts[i], ts[i], pt))
            ts[i] = g2_add(ts[i], ts[i])
            if bit == "1":
                f = f12_mul(f, _line(ts[i], q, pt))
                ts[i] = g2_add(ts[i], q)
    for i, (pt, q) in enumerate(pairs):
        q1 = g2_frob(q)
        q2 = g2_neg(g2_frob(q1))
        f = f12_mul(f, _line(ts[i], q1, pt))
        ts[i] = g2_add(ts[i], q1)
        f = f12_mul(f, _line(ts[i], q2, pt))
        ts[i] = g2_add(ts[i], q2)
    return f


def final_exp(f):
    """f^((p^12 - 1)/r): the easy part (p^6 - 1)(p^2 + 1) by conjugate, inverse and Frobenius, the hard part by plain powering"""
    f = f12_mul(f12_conj(f), f12_inv(f))
    f = f12_mul(f12_frob(f, 2), f)
    return f12_pow(f, HARD)


def final_exp_plain(f):
    return f12_pow(f, FINAL)


def pairing(pt, q):
    return final_exp(miller_loop([(pt, q)]))


def pairing_check(pairs):
    if not all(g1_on_curve(pt) for pt, _ in pairs) or not all(g2_on_curve(q) for _, q in pairs):
        return -1
    return 1 if f12_is_one(final_exp(miller_loop(pairs))) else 0


# ---------------------------------------------------------------- ABI encodings (Montgomery words)
def _mont_words(x):
    m = (x % P) * MONT % P
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def _from_words(ws):
    m = sum(int(w) << (64 * i) for i, w in enumerate(ws))
    return m * pow(MONT, -1, P) % P


def g1_words(pt):
    return [0] * 8 if pt is None else _mont_words(pt[0]) + _mont_words(pt[1])


def g2_words(q):
    if q is None:
        return [0] * 16
    return _mont_words(q[0][0]) + _mont_words(q[0][1]) + _mont_words(q[1][0]) + _mont_words(q[1][1])


def g2_from_words(ws):
    ws = [int(w) for w in ws]
    if not any(ws):
        return None
    c = [_from_words(ws[4 * i: 4 * i + 4]) for i in range(4)]
    return ((c[0], c[1]), (c[2], c[3]))


def gt_words(f):
    out = []
    for c in f12_coeffs(f):
        out += _mont_words(c[0]) + _mont_words(c[1])
    return out


def fr_words(s):
    m = (s % R) * MONT % R
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
