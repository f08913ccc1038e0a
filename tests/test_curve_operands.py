"""CPU: the catalogue of structured curve operands (tests/curve_operands.py) is well formed; its model of the MSM's signed-digit
recoding (scalar_prepare + next_digit of csrc/pz_msm.hip) rebuilds min(s, r - s) from digits in (-2^(c-1), 2^(c-1)] with no carry out of
window 253/c, at every width the library accepts; the scalar catalogue reaches every branch of the recoding at every width the GPU
tests load (the table below is the one DESIGN.md section 15.14 prints); three independent models of G1 -- oracle/pyref.py,
tests/bn254_pairing_ref.py and the C oracle -- agree on the structured points, so the GPU expectations do not rest on one of them."""
import numpy as np
import pytest

from oracle import pyref as PY
from tests import bn254_pairing_ref as B
from tests import curve_operands as CO

# scalars of the catalogue at width c that take each branch of the recoding: (raw digit 2^c - 1 with a carry in -> digit 0,
# digit 2^(c-1) with no carry in, digit 2^(c-1) + 1 (the first value that carries), a carry out of every window below the top one,
# sign fold taken, sign fold not taken)
BRANCH_TABLE = {
    4: (372, 262, 14, 8, 576, 577),
    5: (296, 204, 4, 12, 460, 461),
    8: (182, 124, 4, 12, 289, 290),
    11: (130, 92, 4, 8, 214, 215),
    13: (110, 76, 4, 12, 181, 182),
    15: (90, 64, 4, 12, 154, 155),
    16: (84, 60, 4, 12, 145, 146),
}
CATALOGUE_SIZES = {4: 1153, 5: 921, 8: 579, 11: 429, 13: 363, 15: 309, 16: 291}


def test_moduli_and_the_identity_encoding():
    assert CO.P == PY.FQ_P == B.P and CO.R == PY.FR_R == B.R
    # 3 is a non-residue mod p: x = 0 gives y^2 = 3, so no point has x = 0 and (0, 0) is free to encode the identity
    assert pow(3, (CO.P - 1) // 2, CO.P) == CO.P - 1
    assert CO.sqrt_fq(3) is None and not CO.on_curve((0, 1)) and CO.on_curve(CO.INF)
    # the roots this file relies on
    for a in (1, 2, 3, 4, 9, CO.P - 1, 12345):
        y = CO.sqrt_fq(a)
        assert (y is None) == (pow(a, (CO.P - 1) // 2, CO.P) != 1) and (y is None or y * y % CO.P == a)
        x = CO.cbrt_fq(a)
        assert (x is None) == (pow(a, (CO.P - 1) // 3, CO.P) != 1) and (x is None or pow(x, 3, CO.P) == a)


def test_g1_catalogue_is_what_it_says():
    roots = dict(CO.g1_roots())
    pts = dict(CO.g1_points())
    assert len(CO.g1_roots()) == 19 and len(pts) == 29 and len(set(pts.values())) == 29 and len(CO.g1_pairing_points()) == 20
    for nm, pt in pts.items():
        assert CO.on_curve(pt), nm
        assert CO.neg(pt) in pts.values(), nm
    # the four smallest x, the four largest, the four smallest y: nothing smaller was skipped
    assert [roots[k][0] for k in ("x=1", "x=2", "x=3", "x=5")] == [1, 2, 3, 5]
    assert CO.sqrt_fq(4 ** 3 + 3) is None
    assert [CO.P - roots["x=p-%d" % k][0] for k in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert [roots["y=%d" % k][1] for k in (1, 2, 4, 6)] == [1, 2, 4, 6]
    assert CO.cbrt_fq(3 * 3 - 3) is None and CO.cbrt_fq(5 * 5 - 3) is None
    assert roots["y=2"] == roots["x=1"] == roots["[1]G"] == (1, 2)
    assert roots["[r-1]G"] == CO.neg(CO.G) and roots["[(r+1)/2]G"] == CO.neg(roots["[(r-1)/2]G"])
    # near-p coordinates are really near p
    assert CO.P - CO.neg(roots["y=1"])[1] == 1 and CO.P - roots["x=p-1"][0] == 1


def test_r_times_every_structured_point_is_the_identity():
    """BN254 G1 has prime order r (cofactor 1): every point of the curve, however it was found, is a legal base"""
    for nm, pt in CO.g1_points():
        assert CO.mul(pt, CO.R) == CO.INF, nm
        if pt != CO.INF:
            assert CO.mul(pt, CO.R - 1) == CO.neg(pt), nm


def test_jacobian_forms_describe_the_same_point():
    for nm, pt in CO.g1_points():
        for lam in CO.LAMBDAS:
            X, Y, Z = CO.jacobian(pt, lam)
            assert PY.jac_to_aff((X, Y, Z)) == pt, (nm, lam)
            assert (Z == 0) == (pt == CO.INF) and (X, Y) != (0, 0)
            w = CO.jac_words(pt, lam)
            assert len(w) == 12 and [CO.fq_from_words(w[4 * i: 4 * i + 4]) for i in range(3)] == [X, Y, Z]


def test_scalar_catalogue_shape():
    assert set(CO.SCALAR_CONSTANTS) == {0, 1, 2, CO.R - 1, CO.R - 2, CO.HALF, CO.HALF + 1, CO.HALF - 1, CO.HALF + 2}
    assert (CO.R + 1) // 2 == CO.HALF + 1
    for c in CO.WINDOWS:
        ss = CO.scalars_for(c)
        assert len(ss) == len(set(ss)) == CATALOGUE_SIZES[c], (c, len(ss))
        assert all(0 <= s < CO.R for s in ss) and all((CO.R - s) % CO.R in ss for s in ss)
        for w in range(CO.n_windows(c)):
            for k in (c * w - 1, c * w, c * w + 1):
                for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if k >= 0 else ():
                    assert v >= CO.R or v in ss, (c, k)
        for d in CO.pattern_digits(c):
            v = CO.pattern_scalar(c, d)
            assert v in ss and v <= CO.HALF
            digs = [(v >> (c * w)) & ((1 << c) - 1) for w in range(CO.n_windows(c))]
            lowered = [w for w, x in enumerate(digs) if x != d]
            # only top windows were lowered, and at most two of them
            assert len(lowered) <= 2 and all(w >= CO.n_windows(c) - 2 for w in lowered), (c, d, lowered)
            assert all(x <= d for x in digs)
    assert len(CO.scalars_all()) == 1501


@pytest.mark.parametrize("c", range(4, 17))
def test_recoding_rebuilds_the_scalar(c):
    top = 253 // c
    for s in CO.scalars_all():
        negate, digs, carry = CO.recode(s, c)
        assert len(digs) == top + 1
        assert carry == 0, (hex(s), c)                                # no carry out of window 253/c
        assert sum(d << (c * w) for w, d in enumerate(digs)) == min(s, CO.R - s), (hex(s), c)
        assert all(-(1 << (c - 1)) < d <= (1 << (c - 1)) for d in digs), (hex(s), c)
        assert negate == (s > CO.HALF)
        # the signed value: sum d_w 2^(cw) with the sign folded back is s mod r
        assert (-1 if negate else 1) * sum(d << (c * w) for w, d in enumerate(digs)) % CO.R == s


def test_sign_fold_is_not_what_keeps_the_digits_in_range():
    """how exact the comparison r - s < s has to be (mutation (b)): not at all, for values.  Window 253/c
    starts at bit c (253/c) and r >> that is below 2^(c-1) at every width 4 .. 16, so ANY canonical scalar recodes without a carry
    out of the last window, folded or not: the fold halves the expected top digit, it does not rescue a value.  A comparison that
    ignores the low 32 bits decides wrongly only within 2^32 of r/2, and the digits it then produces are those of the same scalar:
    no test of values can see that mutation, which is why it survives both this suite and the earlier one."""
    for c in range(4, 17):
        assert (CO.R >> (c * (253 // c))) + 1 <= 1 << (c - 1), c
        near_half = [CO.HALF + d for d in (1, 2, 3, 1 << 31, (1 << 32) - 1, 1 << 64)]
        for s in list(CO.scalars_all()) + near_half:
            negate, digs, carry = CO.recode(s, c, fold=False)
            assert not negate and carry == 0, (c, hex(s))
            assert sum(d << (c * w) for w, d in enumerate(digs)) == s
            assert all(-(1 << (c - 1)) < d <= (1 << (c - 1)) for d in digs)
        assert all(CO.recode(s, c)[0] for s in near_half)         # the fold the device does take there


def test_recoding_c16_twin():
    """k_msm_hist / k_msm_scatter / k_msm_scatter_coarse unroll c == 16 with their own arithmetic: d0 = half-limb + carry, carry =
    d0 > 0x8000, magnitude = carry ? 0x10000 - d0 : d0.  The same digits as the general recoding."""
    for s in CO.scalars_all():
        negate, digs, _ = CO.recode(s, 16)
        m = min(s, CO.R - s)
        limbs = [(m >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
        carry = 0
        for w in range(16):
            d0 = ((limbs[w >> 1] >> (16 * (w & 1))) & 0xFFFF) + carry
            carry = 1 if d0 > 0x8000 else 0
            mag = 0x10000 - d0 if carry else d0
            assert mag == abs(digs[w]) and (carry == 1) == (digs[w] < 0 or (digs[w] == 0 and d0 == 0x10000)), (hex(s), w)
        assert carry == 0


def test_branch_table():
    for c in CO.WINDOWS:
        t = CO.branch_table(c)
        assert tuple(t[b] for b in CO.BRANCHES) == BRANCH_TABLE[c], (c, t)
        assert all(v >= 1 for v in t.values()), (c, t)
    # what the named patterns are for, at every width: all digits 2^c - 1 is -1 then zeros under a running carry; 2^(c-1) stays
    # as it is; 2^(c-1) + 1 carries out of every window
    for c in CO.WINDOWS:
        d1, dlo, dh, dh1, dff = CO.pattern_digits(c)
        _, digs, _ = CO.recode(CO.pattern_scalar(c, dff), c)
        assert digs[0] == -1 and digs.count(0) >= CO.n_windows(c) - 3
        assert "carry_in_to_zero" in CO.branches(CO.pattern_scalar(c, dff), c)
        _, digs, _ = CO.recode(CO.pattern_scalar(c, dh), c)
        assert digs.count(dh) >= CO.n_windows(c) - 2 and "half_no_carry" in CO.branches(CO.pattern_scalar(c, dh), c)
        _, digs, _ = CO.recode(CO.pattern_scalar(c, dh1), c)
        assert digs[0] == -(dh - 1) and digs[1:].count(-(dh - 2)) >= CO.n_windows(c) - 4
        assert {"half_plus_one", "carry_through_all"} <= set(CO.branches(CO.pattern_scalar(c, dh1), c))
        # one dense column of either pattern puts nearly every digit in one bucket: |d| = 1 / 2^(c-1) - 2
        _, digs, _ = CO.recode(CO.pattern_scalar(c, d1), c)
        assert digs.count(1) >= CO.n_windows(c) - 2


MODEL_SCALARS = (0, 1, 2, 3, CO.R - 1, CO.HALF, CO.HALF + 1, CO.pattern_scalar(16, 0x8001), CO.pattern_scalar(5, 31), (1 << 253) + 1)


def test_three_models_of_g1_agree_on_the_structured_points(cref):
    b_of = lambda pt: None if pt == CO.INF else pt
    of_b = lambda pt: CO.INF if pt is None else pt
    c_aff = lambda jac: CO.aff_from_words([int(v) for v in cref.g1_normalize(jac)])
    pts = CO.g1_points()
    for nm, pt in pts:
        aff = np.array(CO.aff_words(pt), dtype=np.uint64)
        for k in MODEL_SCALARS:
            want = CO.mul(pt, k % CO.R)
            assert PY.g1_mul(pt, k) == want, (nm, hex(k))
            if k in (0, 2, CO.R - 1, CO.HALF + 1):     # this model inverts at every addition: a few scalars, every point
                assert of_b(B.g1_mul(b_of(pt), k)) == want, (nm, hex(k))
            assert c_aff(cref.g1_mul(aff, k % CO.R)) == want, (nm, hex(k))
    # additions: every structured point with itself (doubling), its negation (cancellation), the identity, G and its neighbour in the list
    for i, (nm, pt) in enumerate(pts):
        for other in (pt, CO.neg(pt), CO.INF, CO.G, pts[(i + 1) % len(pts)][1]):
            want = CO.add(pt, other)
            assert CO.on_curve(want)
            assert PY.g1_add_aff(pt, other) == want, nm
            assert of_b(B.g1_add(b_of(pt), b_of(other))) == want, nm
            for l1, l2 in ((1, 1), (2, CO.P - 1), (CO.LAMBDAS[3], 2)):
                ja = np.array(CO.jac_words(pt, l1), dtype=np.uint64)
                jb = np.array(CO.jac_words(other, l2), dtype=np.uint64)
                assert c_aff(cref.g1_add(ja, jb)) == want, (nm, l1, l2)


def test_g2_catalogue_and_the_twist_point():
    from tests import g2_wire_ref as G2W

    g2 = CO.g2_points()
    assert len(g2) == 9 and g2[-1] == ("identity", None)      # +-1, +-2, +-3, +-(r-1)/2 and the identity
    for nm, q in g2:
        assert B.g2_on_curve(q), nm
        assert G2W.check(q) == 0, nm
    t = CO.twist_point_outside_subgroup()
    assert B.g2_on_curve(t) and G2W.check(t) == 3 and B.g2_mul(t, B.R, reduce=False) is not None
