"""CPU: the algebra behind the quotient's permutation and lookup lines on two cosets, in Python integers.

n = 8, bf = 2 (u = 5 usable rows), three permuted columns in chunks of two (two sets, the last one short), one lookup.  The numerator
of h is Low + l_active D (the gate group is a further summand of the Low kind: degree <= 3n - 3, zero on the domain; it has been on part A
since the gate change and is left out here):

  * D, the y-weighted product lines without l_active, is zero on the active rows of H and equals the d_i computed from the Lagrange
    values on the other rows (row n - 1 reads z(w^0));
  * D's coefficients follow from its values on part A (2n points) and those d_i, and D_2's top two coefficients vanish;
  * h rebuilt from {part A values, d_i} -- Low / Z_H from part A alone, l_active D / Z_H through the three-coset join with the single
    part-B column D_0 + lam D_1 - g^2n D_2 -- equals h from all 4n points of halo2's coset;
  * a product altered on an active row makes D_2's top two coefficients non-zero."""
import random

from oracle import pyref as P

R = P.FR_R
K, BF, CHUNK = 3, 2, 2
N = 1 << K
U = N - (BF + 1)
W = P.fr_omega(K)
W4 = P.fr_omega(K + 2)
G = pow(P.FR_GENERATOR, (R - 1) // 3, R)
DELTA = pow(P.FR_GENERATOR, 1 << P.FR_S, R)
inv = lambda a: pow(a, -1, R)


def idft(vals, shift, root):
    """values at shift * root^i, i < len(vals) -> the coefficients of the polynomial of degree < len(vals) through them"""
    size = len(vals)
    si, ri, ninv = inv(shift), inv(root), inv(size)
    plain = [sum(v * pow(ri, i * j, R) for i, v in enumerate(vals)) * ninv % R for j in range(size)]
    return [c * pow(si, j, R) % R for j, c in enumerate(plain)]


def ev(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def world(seed=0x2c05):
    rng = random.Random(seed)
    rnd = lambda: rng.randrange(R)
    m = 3
    S = -(-m // CHUNK)
    # a permutation of the cells of the active rows (identity on the blinding rows), values constant on its cycles
    cells = [(c, r) for c in range(m) for r in range(U)]
    image = cells[:]
    rng.shuffle(image)
    sigma_of = dict(zip(cells, image))
    val = {}
    for cell in cells:
        if cell in val:
            continue
        v, cur = rnd(), cell
        while cur not in val:
            val[cur] = v
            cur = sigma_of[cur]
    cols = [[val[(c, r)] if r < U else rnd() for r in range(N)] for c in range(m)]
    label = lambda c, r: pow(DELTA, c, R) * pow(W, r, R) % R
    sigma = [[label(*sigma_of[(c, r)]) if r < U else label(c, r) for r in range(N)] for c in range(m)]
    beta, gamma, y = rnd(), rnd(), rnd()
    # the products, by the recurrence; set j starts where set j - 1 stood at row u; rows above u are blinding
    Z, z0 = [], 1
    for j in range(S):
        z = [z0]
        for i in range(U):
            num = den = 1
            for c in range(j * CHUNK, min(m, (j + 1) * CHUNK)):
                num = num * (cols[c][i] + beta * label(c, i) + gamma) % R
                den = den * (cols[c][i] + beta * sigma[c][i] + gamma) % R
            z.append(z[-1] * num % R * inv(den) % R)
        z0 = z[U]
        Z.append(z + [rnd() for _ in range(N - U - 1)])
    assert Z[-1][U] == 1
    # one lookup: inputs from the table, A' sorted, S' a permutation of the table with a' = s' wherever a' changes
    table = [3 * i + 1 for i in range(N)]
    a = [table[rng.randrange(U)] for _ in range(U)] + [rnd() for _ in range(N - U)]
    ap = sorted(a[:U])
    rest = [t for t in table[:U] if t not in ap]
    sp = [ap[i] if i == 0 or ap[i] != ap[i - 1] else rest.pop() for i in range(U)]
    assert sorted(sp) == sorted(table[:U])
    zl = [1]
    for i in range(U):
        zl.append(zl[-1] * (a[i] + beta) % R * (table[i] + gamma) % R * inv((ap[i] + beta) * (sp[i] + gamma) % R) % R)
    assert zl[U] == 1
    ap += [rnd() for _ in range(N - U)]
    sp += [rnd() for _ in range(N - U)]
    zl += [rnd() for _ in range(N - U - 1)]
    return dict(m=m, S=S, cols=cols, sigma=sigma, Z=Z, table=table, a=a, ap=ap, sp=sp, zl=zl, beta=beta, gamma=gamma, y=y)


class Lines:
    """the permutation and lookup lines at any point X, from the coefficient forms"""

    def __init__(self, w):
        self.w = w
        c = lambda v: idft(v, 1, W)
        self.cols, self.sigma, self.Z = [c(v) for v in w["cols"]], [c(v) for v in w["sigma"]], [c(v) for v in w["Z"]]
        self.table, self.a, self.ap, self.sp, self.zl = (c(w[f]) for f in ("table", "a", "ap", "sp", "zl"))
        self.l0 = c([1] + [0] * (N - 1))
        self.llast = c([int(i == U) for i in range(N)])
        self.lact = c([int(i < U) for i in range(N)])

    def d_perm(self, j, X):
        w = self.w
        left, right = ev(self.Z[j], W * X % R), ev(self.Z[j], X)
        for c in range(j * CHUNK, min(w["m"], (j + 1) * CHUNK)):
            v = ev(self.cols[c], X)
            left = left * (v + w["beta"] * ev(self.sigma[c], X) + w["gamma"]) % R
            right = right * (v + w["beta"] * pow(DELTA, c, R) * X + w["gamma"]) % R
        return (left - right) % R

    def d_lookup(self, X):
        w = self.w
        return (ev(self.zl, W * X % R) * (ev(self.ap, X) + w["beta"]) * (ev(self.sp, X) + w["gamma"])
                - ev(self.zl, X) * (ev(self.a, X) + w["beta"]) * (ev(self.table, X) + w["gamma"])) % R

    def all_lines(self, X):
        """[(line value without its row factor, row factor, is a product line)] in halo2's order"""
        S, Z = self.w["S"], self.Z
        l0, ll, la = ev(self.l0, X), ev(self.llast, X), ev(self.lact, X)
        zlast = ev(Z[S - 1], X)
        out = [((1 - ev(Z[0], X)) % R, l0, False), ((zlast * zlast - zlast) % R, ll, False)]
        for j in range(1, S):
            out.append(((ev(Z[j], X) - ev(Z[j - 1], pow(W, U, R) * X % R)) % R, l0, False))      # w^-(bf+1) = w^u
        for j in range(S):
            out.append((self.d_perm(j, X), la, True))
        z, apx, spx = ev(self.zl, X), ev(self.ap, X), ev(self.sp, X)
        out += [((1 - z) % R, l0, False), ((z * z - z) % R, ll, False), (self.d_lookup(X), la, True), ((apx - spx) % R, l0, False),
                ((apx - spx) * (apx - ev(self.ap, inv(W) * X % R)) % R, la, False)]
        return out

    def numerator(self, X):
        acc = 0
        for v, f, _ in self.all_lines(X):
            acc = (acc * self.w["y"] + v * f) % R
        return acc

    def low_and_d(self, X):
        """the two accumulators of the split kernels: both step through every line's power of y"""
        low = dd = 0
        for v, f, product in self.all_lines(X):
            low = (low * self.w["y"] + (0 if product else v * f)) % R
            dd = (dd * self.w["y"] + (v if product else 0)) % R
        return low, dd


def d_rows(w):
    """d_i = D(w^i) on the rows [u, n) from the Lagrange values, with the weights halo2's Horner gives the product lines"""
    S, m, Lk, y, beta, gamma = w["S"], w["m"], 1, w["y"], w["beta"], w["gamma"]
    out = [0] * N
    for i in range(U, N):
        nx = (i + 1) % N                                                  # row n - 1 reads z(w^0)
        acc = 0
        for j in range(S):
            left, right = w["Z"][j][nx], w["Z"][j][i]
            for c in range(j * CHUNK, min(m, (j + 1) * CHUNK)):
                left = left * (w["cols"][c][i] + beta * w["sigma"][c][i] + gamma) % R
                right = right * (w["cols"][c][i] + beta * pow(DELTA, c, R) * pow(W, i, R) + gamma) % R
            acc += (left - right) * pow(y, (S - 1 - j) + 5 * Lk, R)
        l = 0
        dl = w["zl"][nx] * (w["ap"][i] + beta) * (w["sp"][i] + gamma) - w["zl"][i] * (w["a"][i] + beta) * (w["table"][i] + gamma)
        acc += dl * pow(y, 5 * (Lk - 1 - l) + 2, R)
        out[i] = acc % R
    return out


G2N = pow(G, 2 * N, R)
CB = G * W4 % R                      # part B's coset generator
LAM = pow(CB, N, R)
PART_A = [G * pow(W4, 2 * i, R) % R for i in range(2 * N)]
PART_B = [CB * pow(W, i, R) % R for i in range(N)]


def d_coefficients(d_on_a, d_on_h):
    """(D_0, D_1, D_2) from D on part A and on H"""
    ua = idft(d_on_a, G, W4 * W4 % R)
    u_d, d1 = ua[:N], ua[N:]
    v_d = idft(d_on_h, 1, W)
    s = inv(1 - G2N)
    d2 = [(v - a - b) * s % R for v, a, b in zip(v_d, u_d, d1)]
    d0 = [(a - G2N * c) % R for a, c in zip(u_d, d2)]
    return d0, d1, d2


def test_h_from_part_a_and_the_blinding_rows_of_h():
    w = world()
    L = Lines(w)
    zh = lambda X: (pow(X, N, R) - 1) % R
    # the reference: h from all 4n points of halo2's coset
    pts4 = [G * pow(W4, i, R) % R for i in range(4 * N)]
    h_ref = idft([L.numerator(X) * inv(zh(X)) % R for X in pts4], G, W4)
    assert any(h_ref[:3 * N - 3]) and not any(h_ref[3 * N - 3:])
    # D on H: zero on the active rows, the d_i elsewhere
    d_h = d_rows(w)
    for i in range(N):
        assert L.low_and_d(pow(W, i, R))[1] == d_h[i]
        assert (d_h[i] == 0) == (i < U)
    # part A: the two accumulators sum to the numerator
    low_a, d_a = zip(*(L.low_and_d(X) for X in PART_A))
    lact_a = [ev(L.lact, X) for X in PART_A]
    for X, lo, dd, la in zip(PART_A, low_a, d_a, lact_a):
        assert (lo + la * dd) % R == L.numerator(X)
    # D's coefficients; they are the true ones (from 4n points), and D_2's top two vanish
    d0, d1, d2 = d_coefficients(list(d_a), d_h)
    assert d0 + d1 + d2 + [0] * N == idft([L.low_and_d(X)[1] for X in pts4], G, W4)
    assert d2[N - 2:] == [0, 0] and d2[N - 3] != 0
    # Low / Z_H from part A alone: 2n coefficients, the top two zero
    q = idft([lo * inv(zh(X)) % R for X, lo in zip(PART_A, low_a)], G, W4 * W4 % R)
    assert q[2 * N - 2:] == [0, 0]
    # l_active D / Z_H through the three-coset join; part B carries the single column D_0 + lam D_1 - g^2n D_2
    col_b = [(a + LAM * b - G2N * c) % R for a, b, c in zip(d0, d1, d2)]
    ua = idft([la * dd % R * inv(zh(X)) % R for X, la, dd in zip(PART_A, lact_a, d_a)], G, W4 * W4 % R)
    v = idft([ev(col_b, X) * ev(L.lact, X) % R * inv(zh(X)) % R for X in PART_B], CB, W)
    uu, h1 = ua[:N], ua[N:]
    h2 = [(a - c + LAM * b) * inv(2 * G2N) % R for a, b, c in zip(uu, h1, v)]
    h0 = [(a - G2N * c) % R for a, c in zip(uu, h2)]
    h = [(a + b) % R for a, b in zip(h0 + h1, q)] + h2
    assert h == h_ref[:3 * N]


def test_a_product_altered_on_an_active_row_shows_in_d2():
    for which in ("Z", "zl"):
        w = world()
        if which == "Z":
            w["Z"][0][2] = (w["Z"][0][2] + 1) % R
        else:
            w["zl"][3] = (w["zl"][3] + 1) % R
        L = Lines(w)
        d_a = [L.low_and_d(X)[1] for X in PART_A]
        d2 = d_coefficients(d_a, d_rows(w))[2]
        assert d2[N - 2] != 0 and d2[N - 1] != 0, which
