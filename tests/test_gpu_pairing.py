"""GPU: the HIP pairing (csrc/pz_pairing.hip) against the Python restatement (tests/bn254_pairing_ref.py): e(P, Q) word for
word, bilinearity, G2 scalar multiplication, and the batched pairing-product check on 1024 checks."""
import random
import time

import numpy as np
import pytest

from tests import bn254_pairing_ref as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    yield e
    e.close()


class Dev:
    """device buffers of one test, freed at the end"""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def put(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        d = self.eng.dev_alloc(max(a.nbytes, 8))
        self.eng.upload(d, a)
        self.ptrs.append(d)
        return d

    def empty(self, nbytes):
        d = self.eng.dev_alloc(nbytes)
        self.ptrs.append(d)
        return d

    def free(self):
        for d in self.ptrs:
            self.eng.dev_free(d)


@pytest.fixture
def dev(eng):
    d = Dev(eng)
    yield d
    d.free()


def pairing_dev(eng, dev, pts, qs):
    n = len(pts)
    d_gt = dev.empty(n * 48 * 8)
    eng.pairing_dev(dev.put([B.g1_words(p) for p in pts]), dev.put([B.g2_words(q) for q in qs]), n, d_gt)
    return eng.download(d_gt, (n, 48))


def g2_mul_dev(eng, dev, qs, scalars):
    n = len(qs)
    d_out = dev.empty(n * 16 * 8)
    eng.g2_mul_dev(dev.put([B.g2_words(q) for q in qs]), dev.put([B.fr_words(s) for s in scalars]), n, d_out)
    return eng.download(d_out, (n, 16))


def test_pairing_matches_restatement(eng, dev):
    rng = random.Random(11)
    pts, qs = [], []
    for _ in range(6):
        pts.append(B.g1_mul(B.G1, rng.randrange(1, B.R)))
        qs.append(B.g2_mul(B.G2, rng.randrange(1, B.R)))
    pts += [None, B.G1, B.G1]
    qs += [B.G2, None, B.G2]
    got = pairing_dev(eng, dev, pts, qs)
    t0 = time.perf_counter()
    pairing_dev(eng, dev, pts[:1], qs[:1])
    print("\npz_pairing_dev: 1 pairing %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    for i, (p, q) in enumerate(zip(pts, qs)):
        want = B.gt_words(B.pairing(p, q))
        assert [int(v) for v in got[i]] == want, i
    assert [int(v) for v in got[6]] == B.gt_words(B.F12_ONE) and [int(v) for v in got[7]] == B.gt_words(B.F12_ONE)


def test_pairing_bilinear_on_device(eng, dev):
    rng = random.Random(12)
    a, b = rng.randrange(1, B.R), rng.randrange(1, B.R)
    pa, qb = B.g1_mul(B.G1, a), B.g2_mul(B.G2, b)
    got = pairing_dev(eng, dev, [pa, B.g1_mul(B.G1, a * b), B.G1], [qb, B.G2, B.G2])
    assert np.array_equal(got[0], got[1])
    # e(G1, G2)^(ab) from the device's own e(G1, G2), powered in the restatement
    e = B.f12_from_coeffs([(B._from_words(got[2][8 * i: 8 * i + 4]), B._from_words(got[2][8 * i + 4: 8 * i + 8])) for i in range(6)])
    assert B.gt_words(B.f12_pow(e, a * b % B.R)) == [int(v) for v in got[0]]
    assert B.f12_pow(e, B.R) == B.F12_ONE and e != B.F12_ONE


def test_g2_mul_matches_restatement(eng, dev):
    rng = random.Random(13)
    ss = [0, 1, 2, B.R - 1] + [rng.randrange(B.R) for _ in range(8)]
    q = B.g2_mul(B.G2, 0xC0FFEE)
    qs = [q] * len(ss) + [None]
    ss = ss + [5]
    t0 = time.perf_counter()
    got = g2_mul_dev(eng, dev, qs, ss)
    print("\npz_g2_mul_dev: %d multiplications %.1f ms" % (len(ss), (time.perf_counter() - t0) * 1e3))
    for i, (qq, s) in enumerate(zip(qs, ss)):
        want = None if qq is None else B.g2_mul(qq, s)
        assert B.g2_from_words(got[i]) == want, (i, s)
    assert not got[0].any() and not got[-1].any()   # [0] Q and [s] O: the all-zero identity


def test_pairing_check_1024(eng, dev):
    """1024 checks of 2 pairs: e([ab]P, Q) e(-[a]P, [b]Q), half with one scalar perturbed, a few with a point off its curve"""
    rng = random.Random(14)
    n = 1024
    a = [rng.randrange(1, B.R) for _ in range(n)]
    b = [rng.randrange(1, B.R) for _ in range(n)]
    holds = [i % 2 == 0 for i in range(n)]
    ab = [(a[i] * b[i] + (0 if holds[i] else 1 + rng.randrange(1000))) % B.R for i in range(n)]
    # the points come from the device (K1's fixed-base kernel for G1, pz_g2_mul_dev for G2; both held against restatements)
    g1 = eng.g1_fixed_base_mul(np.array([B.fr_words(s) for s in sum(([ab[i], B.R - a[i]] for i in range(n)), [])], dtype=np.uint64))
    g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(n, 2, 8)
    gen = B.g2_words(B.G2)
    qb = g2_mul_dev(eng, dev, [B.G2] * n, b)
    g2 = np.zeros((n, 2, 16), dtype=np.uint64)
    g2[:, 0] = gen
    g2[:, 1] = qb
    want = [1 if h else 0 for h in holds]
    # off the curve: G1 y + 1, G2 y + 1 (canonical coordinates, wrong curve), a non-canonical x
    for i, which in ((3, "g1"), (10, "g2"), (501, "g1"), (1000, "canon")):
        if which == "g1":
            x, y = B._from_words(g1[i, 1, :4]), B._from_words(g1[i, 1, 4:])
            g1[i, 1] = B.g1_words((x, y + 1))
        elif which == "g2":
            q = B.g2_from_words(g2[i, 1])
            g2[i, 1] = B.g2_words((q[0], (q[1][0] + 1, q[1][1])))
        else:
            g1[i, 0, :4] = [0xFFFFFFFFFFFFFFFF] * 3 + [0x3FFFFFFFFFFFFFFF]
        want[i] = -1
    # identities contribute 1: a check of two identity pairs holds, so does one whose only live pair is trivial
    g1[20] = 0
    g2[20] = 0
    want[20] = 1
    d_g1, d_g2 = dev.put(g1), dev.put(g2)
    d_ok = dev.empty(n * 4)
    # one check first (its latency), then the batch
    eng.pairing_check_dev(d_g1, d_g2, 1, 2, d_ok)
    eng.download(d_ok, 1, np.int32)
    t0 = time.perf_counter()
    eng.pairing_check_dev(d_g1, d_g2, 1, 2, d_ok)
    one = eng.download(d_ok, 1, np.int32)
    t1 = time.perf_counter()
    eng.pairing_check_dev(d_g1, d_g2, n, 2, d_ok)
    got = eng.download(d_ok, n, np.int32)
    t2 = time.perf_counter()
    print("\npz_pairing_check_dev (2 pairs): 1 check %.1f ms, %d checks %.1f ms (%.0f checks/s)"
          % ((t1 - t0) * 1e3, n, (t2 - t1) * 1e3, n / (t2 - t1)))
    assert one[0] == want[0]
    assert got.tolist() == want


@pytest.mark.parametrize("m", [1, 3, 5])
def test_pairing_check_pairs_and_ragged_count(eng, dev, m):
    """pz_pairing_check_dev beyond the verifier's one use (2 pairs): pairs_per_check in {1, 3, 5}, n_checks in {1, 63, 65} (below, at
    and past the 64-lane workgroup; the kernel strides its per-pair state by n_checks).  Points of known logs, [a_j] G from K1's
    fixed-base kernel and [b_j] G2 from pz_g2_mul_dev; the expected result in integers: 1 exactly when sum_j a_j b_j == 0 (mod r)."""
    rng = random.Random(15 + m)
    for n in (1, 63, 65):
        a = [[rng.randrange(1, B.R) for _ in range(m)] for _ in range(n)]
        b = [[rng.randrange(1, B.R) for _ in range(m)] for _ in range(n)]
        for i in range(0, n, 2):                 # about half the checks hold: the last a_j solved (m = 1: only the identity solves it)
            a[i][m - 1] = -sum(a[i][j] * b[i][j] for j in range(m - 1)) * pow(b[i][m - 1], -1, B.R) % B.R
        if n > 3 and m > 1:
            # check 1: every pair has an identity on one side (G1, G2 or both): each contributes 1 and the check holds trivially
            a[1] = [0, rng.randrange(1, B.R)] + [0] * (m - 2)
            b[1] = [rng.randrange(1, B.R), 0] + [0] * (m - 2)
            # check 2: one live pair e([a] G, [b] G2) with a b != 0 next to identity pairs: must be 0, not 1
            a[2] = [0] * (m - 1) + [rng.randrange(1, B.R)]
            b[2] = [0] * (m - 1) + [rng.randrange(1, B.R)]
            # check 4: the live pair is trivial on the G1 side only
            a[4] = [0] * m
        want = [1 if sum(x * y for x, y in zip(a[i], b[i])) % B.R == 0 else 0 for i in range(n)]
        if m == 1:                               # one pair: a live pair is 0, an identity pair is 1
            assert want == [1 if i % 2 == 0 else 0 for i in range(n)] and all(a[i][0] == 0 for i in range(0, n, 2))
        else:
            assert want[0] == 1 and (n < 3 or (want[1], want[2], want[3], want[4]) == (1, 0, 0, 1))
        if n == 65:
            a[64][m - 1] = rng.randrange(1, B.R)
        g1 = eng.g1_fixed_base_mul(np.array([B.fr_words(s) for row in a for s in row], dtype=np.uint64))
        g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(n, m, 8)
        g2 = g2_mul_dev(eng, dev, [B.G2] * (n * m), [s for row in b for s in row]).reshape(n, m, 16)
        assert not g1[a_is_zero(a)].any() and not g2[a_is_zero(b)].any()      # log 0 is the all-zero identity
        if n == 65:                              # a point off its curve in the last pair of check 64: -1 for that check alone
            x, y = B._from_words(g1[64, m - 1, :4]), B._from_words(g1[64, m - 1, 4:])
            g1[64, m - 1] = B.g1_words((x, (y + 1) % B.P))
            want[64] = -1
        d_ok = dev.empty(n * 4)
        eng.upload(d_ok, np.full(n, 7, dtype=np.int32))
        eng.pairing_check_dev(dev.put(g1), dev.put(g2), n, m, d_ok)
        assert eng.download(d_ok, n, np.int32).tolist() == want, (m, n)


def a_is_zero(rows):
    return np.array([[v == 0 for v in row] for row in rows], dtype=bool)
