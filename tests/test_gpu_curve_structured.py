"""GPU: the curve stack -- Fq in 29-bit limbs, G1 in XYZZ, the MSM's recoding, sort, folds and trees, G2 and the pairing -- on the
structured operands of tests/curve_operands.py.  One Engine, no subprocesses.  Every expected value is a
Python integer or a point from Python point arithmetic (oracle/pyref.py, tests/bn254_pairing_ref.py, tests/curve_operands.py,
tests/wire_ref.py); none comes from another device call -- MSM results leave the device as Jacobian words and are normalised in
Python.  Every comparison is exact."""
import collections
import random
import time

import numpy as np
import pytest

from oracle import pyref as PY
from tests import bn254_pairing_ref as B
from tests import curve_operands as CO
from tests import wire_ref as W

pytestmark = pytest.mark.gpu

R = CO.R
G = CO.G


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

    def put(self, arr, dtype=np.uint64):
        a = np.ascontiguousarray(arr, dtype=dtype)
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
        self.ptrs = []


@pytest.fixture
def dev(eng):
    d = Dev(eng)
    yield d
    d.free()


def words(rows):
    return np.array(rows, dtype=np.uint64)


def aff_of_jac_words(row):
    X, Y, Z = (CO.fq_from_words(row[4 * i: 4 * i + 4]) for i in range(3))
    return PY.jac_to_aff((X, Y, Z))


def aff_of_words(row):
    return CO.aff_from_words([int(v) for v in row])


def log_point(e):
    e %= R
    return PY.g1_mul(G, e) if e else CO.INF


def run_msm(eng, dev, cref, tb, cols, win_lo=0, win_hi=None, density=None):
    """one pz_msm_g1_dev_ex launch over equal-length columns of integer scalars -> the affine result per column, normalised in Python.
    eng.sync() raises if a scatter position check fired (PZ_ERR_ASYNC)."""
    nc, n = len(cols), len(cols[0])
    assert all(len(c) == n for c in cols)
    sw = cref.fr_ints_to_mont([x for c in cols for x in c]).reshape(nc, n, 4)
    d_s, d_o = dev.put(sw), dev.empty(nc * 96)
    eng.upload(d_o, np.full((nc, 12), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
    eng.msm_dev(tb, d_s, nc, n, 4 * n, d_o, win_lo, win_hi, density)
    eng.sync()
    out = eng.download(d_o, (nc, 12))
    dev.free()
    return [aff_of_jac_words([int(v) for v in row]) for row in out]


def rotated(seq, k, n):
    """n entries of seq from position k on, cyclically"""
    L = len(seq)
    return [seq[(k + i) % L] for i in range(n)]


# ------------------------------------------------------------------------------------------ 1. the fixed-base kernel
@pytest.mark.parametrize("part", range(4))
def test_fixed_base_mul_on_the_scalar_catalogue(eng, cref, part):
    ss = CO.scalars_all()[part::4]
    got = eng.g1_fixed_base_mul(cref.fr_ints_to_mont(list(ss)))
    for s, row in zip(ss, got):
        assert aff_of_words(row) == PY.g1_mul(G, s), hex(s)


# ------------------------------------------------------------------------------------------ 2. the recoding through the MSM
WALK_S, WALK_T = 0x2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F7081, 0x1F2E3D4C5B6A79887766554433221100FFEEDDCCBBAA99


def walk_expected(col):
    return log_point(sum(k * (WALK_S + i * WALK_T) for i, k in enumerate(col)))


@pytest.fixture(scope="module")
def walk512(cref):
    return cref.walk_bases(512, WALK_S, WALK_T)


@pytest.mark.parametrize("ncols", [1, 8, 9, 17])
@pytest.mark.parametrize("c", CO.WINDOWS)
def test_msm_recoding_on_the_scalar_catalogue(eng, dev, cref, walk512, c, ncols):
    """the whole catalogue of width c in columns of n scalars (509 or 251: odd, below the 512 bases of the table), launched ncols columns
    at a time -- the few-column path (1), its upper edge (8), the batch path at its lower edge (9) and above (17); a launch the
    catalogue does not fill takes rotated copies, so every scalar also meets other bases"""
    cat = CO.scalars_for(c)
    n = 509 if len(cat) >= 509 else 251
    chunks = [rotated(cat, k, n) for k in range(0, len(cat), n)]
    assert set(x for col in chunks for x in col) == set(cat)
    while len(chunks) % ncols:
        chunks.append(rotated(cat, 37 * len(chunks) + 11, n))
    tb = eng.load_bases(walk512, window_bits=c)
    try:
        assert tb.n_windows == CO.n_windows(c)
        for l0 in range(0, len(chunks), ncols):
            cols = chunks[l0: l0 + ncols]
            got = run_msm(eng, dev, cref, tb, cols)
            for j, col in enumerate(cols):
                assert got[j] == walk_expected(col), (c, ncols, l0 + j)
    finally:
        tb.free()


def _density16(col):
    nz = sum(sum(1 for d in CO.recode(s, 16)[1] if d) for s in col)
    return nz / (16.0 * len(col))


@pytest.mark.parametrize("density", ["auto", "dense", "sparse"])
def test_msm_dense_launch_with_one_bucket_holding_a_column(eng, dev, cref, walk512, density):
    """c = 16, 9 columns, every column with at least 0.4 of its digits non-zero, so that the device picks the two-step scatter by
    itself.  Columns 0, 1: every window's digit 1 (bucket 1 holds 16 n entries); columns 2, 3: every window 0x8001, which recodes to
    -0x7fff, then -0x7ffe under a running carry in 14 windows, then the lowered top window: bucket 0x7ffe holds 14 n of the 16 n
    entries -- the worst skew for the coarse step's cursors.  Odd columns negate every second scalar (the sign fold, the same
    buckets).  The others: dense catalogue patterns of every width and seeded full-width scalars."""
    import paillier_halo2_amd as pz

    n = 509
    rng = random.Random(1514)
    ones, h1 = CO.pattern_scalar(16, 1), CO.pattern_scalar(16, 0x8001)
    assert CO.recode(ones, 16)[1] == [1] * 16
    assert [abs(d) for d in CO.recode(h1, 16)[1]].count(0x7FFE) == 14
    dense_patterns = [s for c in CO.WINDOWS for d in CO.pattern_digits(c) for s in (CO.pattern_scalar(c, d),) if _density16([s]) >= 0.5]
    assert len(dense_patterns) >= 20
    cols = [[ones] * n, [ones if i % 2 else R - ones for i in range(n)], [h1] * n, [h1 if i % 2 else R - h1 for i in range(n)],
            rotated(dense_patterns, 0, n), [R - s for s in rotated(dense_patterns, 5, n)]]
    for j in range(3):
        cols.append([rng.randrange(R) if i % 3 else dense_patterns[(i + j) % len(dense_patterns)] for i in range(n)])
    assert len(cols) == 9 and all(_density16(col) >= 0.4 for col in cols)
    tb = eng.load_bases(walk512, window_bits=16)
    try:
        hint = {"auto": None, "dense": pz.MSM_DENSE, "sparse": pz.MSM_SPARSE}[density]
        got = run_msm(eng, dev, cref, tb, cols, density=hint)      # run_msm's eng.sync() raises if a position check fired
        for j, col in enumerate(cols):
            assert got[j] == walk_expected(col), (density, j)
    finally:
        tb.free()


# ------------------------------------------------------------------------------------------ 3. structured bases
def _structured_base_set(n):
    """[(point, root index, coefficient)]: the identity at 0, n/2 and n - 1, every structured point and negation, the rest +-[a] S"""
    roots = []
    for _, pt in CO.g1_roots():
        if pt not in roots:
            roots.append(pt)
    index = {}
    for i, pt in enumerate(roots):
        index[pt] = (i, 1)
        index.setdefault(CO.neg(pt), (i, -1))
    slots = [None] * n
    for i in (0, n // 2, n - 1):
        slots[i] = (CO.INF, 0, 0)
    free = [i for i in range(n) if slots[i] is None]
    pts = [pt for _, pt in CO.g1_points() if pt != CO.INF]
    for pt in pts:
        i = free.pop(0)
        slots[i] = (pt,) + index[pt]
    small = {}
    for k, i in enumerate(free):
        ri, a = k % len(roots), 2 + (k // len(roots)) % 7
        sign = -1 if (k // 3) % 2 else 1
        if (ri, a) not in small:
            small[(ri, a)] = CO.mul(roots[ri], a)
        pt = small[(ri, a)]
        slots[i] = (pt if sign > 0 else CO.neg(pt), ri, sign * a)
    assert all(CO.on_curve(s[0]) for s in slots)
    return roots, slots


@pytest.fixture(scope="module")
def structured_bases():
    roots, slots = _structured_base_set(256)
    arr = words([CO.aff_words(s[0]) for s in slots])
    assert not arr[0].any() and not arr[128].any() and not arr[255].any()
    return roots, slots, arr


@pytest.mark.parametrize("ncols", [1, 9])
@pytest.mark.parametrize("c", [5, 11, 16])
def test_msm_over_structured_bases(eng, dev, cref, structured_bases, c, ncols):
    """bases with coordinates 1, 2, p - 1, p - 2 ..., P next to -P, identities at both ends and in the middle; the expected value is
    sum over the roots S of [sum_i k_i a_i] S in Python point arithmetic (the roots' mutual logs are not known)"""
    roots, slots, arr = structured_bases
    n = len(slots)
    cat = CO.scalars_for(c)
    cols = [rotated(cat, 101 * j, n) for j in range(ncols)]
    tb = eng.load_bases(arr, window_bits=c)
    try:
        got = run_msm(eng, dev, cref, tb, cols)
    finally:
        tb.free()
    for j, col in enumerate(cols):
        coef = [0] * len(roots)
        for k, (_, ri, a) in zip(col, slots):
            coef[ri] = (coef[ri] + k * a) % R
        want = CO.INF
        for e, s in zip(coef, roots):
            want = PY.g1_add_aff(want, PY.g1_mul(s, e))
        assert got[j] == want, (c, ncols, j)


# ------------------------------------------------------------------------------------------ 4. the folds at their thresholds
MSM_CHUNK_MIN, MSM_CHUNK_MAX, MSM_HEAVY, MSM_MEDIUM, MSM_SLICE_MAX_COLS, MSM_FEW_SMALL = 16, 256, 24, 1024, 8, 32


def msm_chunk_for(n_cols, digits_per_col, window_bits):
    """pz_msm.hip's msm_chunk_for restated: entries one lane accumulates for one bucket work item"""
    if n_cols <= MSM_SLICE_MAX_COLS:
        ch = 0.79 * (digits_per_col / float(1 << (window_bits - 1))) ** 0.63
        c32 = MSM_CHUNK_MIN if ch < 24.0 else 32 * int((ch + 16.0) / 32.0)
        return min(c32, MSM_CHUNK_MAX)
    want = (n_cols * digits_per_col) >> 18
    chunk = MSM_CHUNK_MIN
    while chunk < MSM_CHUNK_MAX and chunk * 2 <= want:
        chunk *= 2
    return chunk


def chunks_of(entries, chunk):
    """k_msm_scan / k_msm_items_few: work items (partial sums to fold) of a bucket with `entries` entries"""
    return -(-entries // chunk)


FOLD_N_BIG = 16400
FOLD_S0 = 0x123456789ABCDEF0FEDCBA9876543210F0E1D2C3B4A5968778695A4B3C2D1E
FAMILIES = ("equal", "alternating", "walk")
BUCKET_SETS = ((1,), (0x8000,), (0x7FFF, 2), (3, 0x8000, 0x4000), (0x7FFE, 0x8000, 1))
RUNS = (1, 2, 16, 256, 1024, 3, 1 << 20, 2048, 4096)    # sign runs of the alternating family, per column


def family_logs(family, n):
    if family == "equal":
        return [FOLD_S0] * n
    if family == "alternating":
        return [FOLD_S0 if i % 2 == 0 else R - FOLD_S0 for i in range(n)]
    return [1 + i for i in range(n)]


@pytest.fixture(scope="module")
def fold_tables(eng, cref):
    """c = 16 tables of FOLD_N_BIG bases per family: all equal; P, -P alternating; G, 2G, 3G ..."""
    p0 = PY.g1_mul(G, FOLD_S0)
    tabs = {}
    for family in FAMILIES:
        if family == "walk":
            arr = cref.walk_bases(FOLD_N_BIG, 1, 1)
        else:
            pair = words([CO.aff_words(p0), CO.aff_words(p0 if family == "equal" else CO.neg(p0))])
            arr = np.ascontiguousarray(np.tile(pair, (FOLD_N_BIG // 2, 1)))
        assert arr.shape == (FOLD_N_BIG, 8)
        tabs[family] = eng.load_bases(arr, window_bits=16)
    yield tabs
    for tb in tabs.values():
        tb.free()


def fold_column(family, m, n, j, chunk):
    """a column of n short scalars (|s| <= 2^15: one digit, window 0) whose chosen buckets hold exactly m chunks -- 16 m entries
    (even j) or 16 (m - 1) + 1 (odd j) -- and whose other scalars fall into single-chunk buckets 100 .. 149 or are zero.
    equal: one sign per bucket, so every partial sum of a bucket is the same point and every fold addition is a doubling.
    alternating: the effective sign of entry i (scalar sign times base sign) changes every RUNS[j] entries: at run 1 and 2 the
    partial sums are the identity or +-[d] P, at longer runs mixed multiples, and at 1024 and above (whole slices of the sort, whose
    order within a bucket is fixed) they are +-[16 d] P in long stretches: the fold doubles, then cancels to the identity, then
    goes on from the identity.
    walk: signs by a fixed pattern over G, 2G, 3G ..."""
    v = chunk * m if j % 2 == 0 else chunk * (m - 1) + 1
    digs = BUCKET_SETS[j % len(BUCKET_SETS)]
    digs = digs[: max(1, min(len(digs), n // v))]
    assert v * len(digs) <= n
    col, pos = [], 0
    for bi, d in enumerate(digs):
        for i in range(pos, pos + v):
            if family == "equal":
                minus = (bi + j) % 2 == 1
            elif family == "alternating":
                eff_minus = ((i - pos) // RUNS[j % len(RUNS)]) % 2 == 1
                minus = eff_minus != (i % 2 == 1)
            else:
                minus = (i * 7 + j) % 3 == 0
            col.append(R - d if minus else d)
        pos += v
    col += [100 + (i % 50) if i - pos < 50 * chunk else 0 for i in range(pos, n)]
    # the restated scan: entries per bucket of window 0 and the chunk counts relied on
    mags = collections.Counter(min(s, R - s) for s in col if s)
    assert all(0 < k <= 0x8000 for k in mags)
    for d in digs:
        assert chunks_of(mags[d], chunk) == m, (d, mags[d])
    assert all(chunks_of(cnt, chunk) == 1 for k, cnt in mags.items() if k not in digs)
    return col


def fold_expected(family, col):
    logs = family_logs(family, len(col))
    return log_point(sum(k * l for k, l in zip(col, logs)))


@pytest.mark.parametrize("m", [1, 2, 24, 25, 32, 33, 1024, 1025])
@pytest.mark.parametrize("family", FAMILIES)
def test_msm_batch_folds_at_their_thresholds(eng, dev, cref, fold_tables, family, m):
    """9 columns at c = 16 whose chosen buckets hold exactly m chunks: 1 (no fold), 2 and 24 (k_msm_bucket_sum's serial fold, its
    last size), 25, 32, 33 and 1024 (k_msm_medium_sum's 32-lane groups, its last size), 1025 (k_msm_heavy_sum); the results then pass
    k_msm_reduce_l1 and three levels of k_msm_combine_quad.  Once over window 0 alone (win_lo = 0, win_hi = 1), once over all 16
    windows of the same short scalars."""
    ncols = 9
    n = 2048 if m <= 33 else FOLD_N_BIG
    chunk = msm_chunk_for(ncols, n, 16)
    assert chunk == 16 and msm_chunk_for(ncols, 16 * n, 16) == 16      # the one-window launch and the 16-window launch
    assert (m > MSM_HEAVY) == (m >= 25) and (m > MSM_MEDIUM) == (m == 1025)
    cols = [fold_column(family, m, n, j, chunk) for j in range(ncols)]
    want = [fold_expected(family, col) for col in cols]
    tb = fold_tables[family]
    for lo, hi in ((0, 1), (0, None)):
        got = run_msm(eng, dev, cref, tb, cols, win_lo=lo, win_hi=hi)
        assert got == want, (family, m, lo, hi, [j for j in range(ncols) if got[j] != want[j]])


@pytest.mark.parametrize("m", [32, 33, 1024, 1025])
@pytest.mark.parametrize("family", FAMILIES)
def test_msm_single_column_folds_at_their_thresholds(eng, dev, cref, fold_tables, family, m):
    """the few-column path on the same columns, one per launch: k_msm_fold_few's 4-lane arm (up to 32 chunks), its 32-lane arm (33 ..
    1024) and k_msm_heavy_few (1025)"""
    n = 2048 if m <= 33 else FOLD_N_BIG
    chunk = msm_chunk_for(1, 16 * n, 16)
    assert chunk == 16 and msm_chunk_for(1, n, 16) == 16
    assert (m > MSM_FEW_SMALL) == (m >= 33)
    tb = fold_tables[family]
    for j in (0, 1, 3):
        col = fold_column(family, m, n, j, chunk)
        got = run_msm(eng, dev, cref, tb, [col])
        assert got[0] == fold_expected(family, col), (family, m, j)


@pytest.mark.parametrize("c", [9, 13])
@pytest.mark.parametrize("family", FAMILIES)
def test_msm_batch_tree_levels_with_empty_buckets(eng, dev, cref, family, c):
    """9 columns of 2^10 scalars at c = 9 (256 buckets: one level above k_msm_reduce_l1) and c = 13 (4096 buckets: two levels): window
    boundary scalars 2^k, 2^k +- 1 and the digit patterns leave most buckets empty, so the radix-16 tree adds identities, equal points
    (a doubling in x29_add_quad) and opposite points"""
    n, ncols = 1 << 10, 9
    logs = family_logs(family, n)
    if family == "walk":
        arr = cref.walk_bases(n, 1, 1)
    else:
        p0 = PY.g1_mul(G, FOLD_S0)
        arr = np.ascontiguousarray(np.tile(words([CO.aff_words(p0), CO.aff_words(p0 if family == "equal" else CO.neg(p0))]), (n // 2, 1)))
    src = CO.boundary_scalars(c) + [CO.pattern_scalar(c, d) for d in CO.pattern_digits(c)]
    src = src + [R - s for s in src if s]
    cols = [rotated(src, 131 * j, n) for j in range(ncols)]
    cols[7] = [1 << (c - 1)] * n                                   # one bucket, the last one, in window 0
    cols[8] = [(1 << (c - 1)) if i % 2 else R - 1 for i in range(n)]   # the last bucket and bucket 1 with the opposite sign
    tb = eng.load_bases(arr, window_bits=c)
    try:
        got = run_msm(eng, dev, cref, tb, cols)
    finally:
        tb.free()
    for j, col in enumerate(cols):
        assert got[j] == log_point(sum(k * l for k, l in zip(col, logs))), (family, c, j)


# ------------------------------------------------------------------------------------------ 5. sums and normalisation of hand-made Jacobian words
def _sum_cases():
    """[(name, [(point, lambda)], expected affine point)]"""
    L = CO.LAMBDAS
    pts = [pt for _, pt in CO.g1_points()]
    cases = []
    for i, (nm, p) in enumerate(CO.g1_points()):
        q, q2 = pts[(i + 3) % len(pts)], pts[(i + 7) % len(pts)]
        for a, b in ((0, 1), (1, 2), (2, 3), (3, 0), (2, 2)):
            cases.append(("%s doubled under %d,%d" % (nm, a, b), [(p, L[a]), (p, L[b])], CO.add(p, p)))
            cases.append(("%s cancelled under %d,%d then two more" % (nm, a, b), [(p, L[a]), (CO.neg(p), L[b]), (q, L[b]), (q2, L[a])],
                          CO.add(q, q2)))
        # Z = 0 over non-zero X and Y at the start, in the middle and at the end; an identity mid-chain after a cancellation
        cases.append((nm + " with Z = 0 entries", [(CO.INF, L[3]), (p, L[1]), (CO.INF, L[2]), (q, L[3]), (CO.INF, L[1])], CO.add(p, q)))
        cases.append((nm + " identity mid-chain", [(p, L[2]), (CO.neg(p), L[3]), (CO.INF, L[1]), (p, L[1]), (p, L[3])], CO.add(p, p)))
    cases.append(("all identity", [(CO.INF, l) for l in L] * 2, CO.INF))
    cases.append(("one identity", [(CO.INF, L[3])], CO.INF))
    return cases


def test_g1_sum_on_hand_made_jacobian_words(eng, dev):
    """k_g1_sum only ever saw points the device produced: here P under two different Z (the doubling branch of x29_add, found through
    U1 == U2 and S1 == S2 rather than equal words), P and -P under different Z, Z = 0 with garbage X and Y, an identity mid-chain"""
    cases = _sum_cases()
    for k, (nm, terms, want) in enumerate(cases):
        jw = words([CO.jac_words(pt, lam) for pt, lam in terms])
        got = eng.g1_sum(jw)
        assert aff_of_jac_words([int(v) for v in got]) == want, nm
        if k % 5 == 0 or len(terms) != 2:        # the device-pointer form on a share of the list
            d_o = dev.empty(96)
            eng.g1_sum_dev(dev.put(jw), len(terms), d_o)
            assert aff_of_jac_words([int(v) for v in eng.download(d_o, 12)]) == want, nm
            dev.free()


def test_g1_normalize_every_structured_point_under_every_z(eng):
    rows, want = [], []
    for nm, pt in CO.g1_points():
        for lam in CO.LAMBDAS:
            rows.append(CO.jac_words(pt, lam))
            want.append(CO.aff_words(pt))
    got = eng.g1_normalize(words(rows))
    assert got.tolist() == want                                  # word for word: canonical Montgomery coordinates, the identity all zero


# ------------------------------------------------------------------------------------------ 6. the wire form
def test_g1_wire_and_curve_check_on_structured_points(eng, dev):
    pts = [pt for _, pt in CO.g1_points()]
    arr = words([CO.aff_words(pt) for pt in pts])
    want = b"".join(W.compress(None if pt == CO.INF else pt) for pt in pts)
    assert eng.g1_compress(arr).tobytes() == want
    back, st = eng.g1_decompress(want)
    assert st.tolist() == [0] * len(pts) and back.tolist() == arr.tolist()
    assert eng.g1_check_dev(dev.put(arr), len(pts)) == 0
    # encodings next to the structured ones that must be refused, each with the reference's status: x with no y (4 and the largest
    # such x below p), x = 0 with the sign bit, x = p and x = p + 1 (not canonical), bit 254 set; then x = 2 with either sign
    x_hi = next(CO.P - k for k in range(1, 64) if CO.sqrt_fq((CO.P - k) ** 3 + 3) is None)
    bad = []
    for x, sign in ((4, 0), (x_hi, 1), (0, 1), (CO.P, 0), (CO.P + 1, 1), (1 | 1 << 254, 0), (2, 0), (2, 1)):
        bad.append((x | sign << 255).to_bytes(32, "little"))
    ref = [W.decompress(b) for b in bad]
    assert [s for s, _ in ref] == [2, 2, 2, 1, 1, 1, 0, 0]
    back, st = eng.g1_decompress(b"".join(bad))
    assert st.tolist() == [s for s, _ in ref]
    assert back.tolist() == [CO.aff_words(CO.INF if pt is None else pt) for _, pt in ref]
    # off the curve by one in a structured coordinate: counted by the curve check, every one of them
    off = [(1, 3), (2, 2), (CO.P - 1, 1), (0, 1), (1, 0), (CO.P - 2, CO.P - 1)]
    assert not any(CO.on_curve(pt) for pt in off)
    mixed = words([CO.aff_words(pt) for pt in pts[:5] + off + pts[5:]])
    assert eng.g1_check_dev(dev.put(mixed), mixed.shape[0]) == len(off)


# ------------------------------------------------------------------------------------------ 7. G2 multiples
def _g2_scalars(ks):
    out = list(CO.SCALAR_CONSTANTS)
    for k in ks:
        out += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    assert all(0 <= s < R for s in out)
    return out


# constants and c = 16 window boundaries: 36 multiplications of G2 (boundaries of windows 1, 2 and 15, each k - 1, k, k + 1), 24 of
# [0xC0FFEE] G2 (windows 1, 8, 15 and the top bits 252, 253) -- 60 reference multiplications in all
G2_CASES = {"G2": (1, (15, 16, 17, 31, 32, 33, 239, 240, 241)), "C0FFEE": (0xC0FFEE, (16, 128, 240, 252, 253))}


@pytest.mark.parametrize("base", sorted(G2_CASES))
def test_g2_mul_on_structured_scalars(eng, dev, base):
    k, ks = G2_CASES[base]
    q = B.g2_mul(B.G2, k)
    ss = _g2_scalars(ks)
    assert len(ss) == {"G2": 36, "C0FFEE": 24}[base]
    d_out = dev.empty(len(ss) * 128)
    eng.g2_mul_dev(dev.put([B.g2_words(q)] * len(ss)), dev.put([B.fr_words(s) for s in ss]), len(ss), d_out)
    got = eng.download(d_out, (len(ss), 16))
    for s, row in zip(ss, got):
        assert B.g2_from_words(row) == B.g2_mul(q, s), (base, hex(s))


@pytest.fixture(scope="module")
def g2_cat():
    return CO.g2_points()


def test_g2_check_on_the_catalogue_and_the_twist_point(eng, g2_cat):
    t = CO.twist_point_outside_subgroup()
    arr = words([B.g2_words(q) for _, q in g2_cat] + [B.g2_words(t)])
    assert eng.g2_check(arr).tolist() == [0] * len(g2_cat) + [3]


# ------------------------------------------------------------------------------------------ 8. the pairing, word for word
@pytest.mark.parametrize("kname", ["3", "(r-1)/2"])
def test_pairing_of_every_structured_g1_point(eng, dev, g2_cat, kname):
    """e(S, [k] G2) for the 20 points of g1_pairing_points and two k: 40 reference pairings in the two cases of this test"""
    q = dict(g2_cat)["[%s]G2" % kname]
    pts = CO.g1_pairing_points()
    d_gt = dev.empty(len(pts) * 48 * 8)
    eng.pairing_dev(dev.put([CO.aff_words(pt) for _, pt in pts]), dev.put([B.g2_words(q)] * len(pts)), len(pts), d_gt)
    got = eng.download(d_gt, (len(pts), 48))
    for (nm, pt), row in zip(pts, got):
        want = B.gt_words(B.pairing(None if pt == CO.INF else pt, q))
        assert [int(v) for v in row] == want, (nm, kname)


# ------------------------------------------------------------------------------------------ 9. pairing products
def _check_launch(eng, dev, checks):
    """checks: [[(g1 affine, g2 point or None)] * m] -> the int32 verdicts"""
    n, m = len(checks), len(checks[0])
    assert all(len(ch) == m for ch in checks)
    g1 = words([CO.aff_words(p) for ch in checks for p, _ in ch])
    g2 = words([B.g2_words(q) for ch in checks for _, q in ch])
    d_ok = dev.empty(n * 4)
    eng.upload(d_ok, np.full(n, 7, dtype=np.int32))
    eng.pairing_check_dev(dev.put(g1), dev.put(g2), n, m, d_ok)
    return eng.download(d_ok, n, np.int32).tolist()


def test_pairing_check_cancellations_and_repeats(eng, dev, g2_cat):
    """65 checks of 2 pairs over every structured S and the G2 catalogue: (S, Q)(-S, Q) and (S, Q)(S, -Q) are 1; (S, Q)(S, Q) is
    e(S, Q)^2, which is 1 only for an identity (the order r is odd).  Lane 63 -- the last of the first workgroup -- holds a check
    whose pairs are all identities, lane 64 -- alone in the second -- a live check that fails; then the two swap."""
    pts = [pt for _, pt in CO.g1_points()]
    qs = [q for _, q in g2_cat if q is not None]
    checks, want = [], []
    for i in range(63):
        s, q = pts[i % len(pts)], qs[i % len(qs)]
        kind = (i // len(pts) + i) % 3
        if kind == 0:
            checks.append([(s, q), (CO.neg(s), q)])
            want.append(1)
        elif kind == 1:
            checks.append([(s, q), (s, B.g2_neg(q))])
            want.append(1)
        else:
            checks.append([(s, q), (s, q)])
            want.append(1 if s == CO.INF else 0)
    assert want.count(0) >= 15 and want.count(1) >= 40
    idle = [(CO.INF, qs[1]), (pts[4], None)]
    live = [(pts[9], qs[2]), (pts[9], qs[2])]
    assert _check_launch(eng, dev, checks + [idle, live]) == want + [1, 0]
    assert _check_launch(eng, dev, checks + [live, [(CO.INF, None), (CO.INF, None)]]) == want + [0, 1]


def test_pairing_check_the_same_pair_four_times(eng, dev, g2_cat):
    """65 checks of 4 pairs: (S, Q) three times and a fourth solved to cancel them -- ([r - 3] S, Q), or (S, [r - 3] Q) for a few Q --
    is 1; with [r - 2] S it is e(S, Q), not 1"""
    pts = [pt for _, pt in CO.g1_points()]
    qs = [q for _, q in g2_cat if q is not None]
    q_m3 = {i: B.g2_mul(qs[i], R - 3) for i in (0, 3, 6)}
    checks, want, solved_in_g2 = [], [], 0
    for i in range(65):
        s, qi = pts[(i * 5) % len(pts)], i % len(qs)
        q = qs[qi]
        if i % 4 == 3:
            checks.append([(s, q)] * 3 + [(CO.mul(s, R - 2), q)])
            want.append(1 if s == CO.INF else 0)
        elif qi in q_m3 and i % 3 == 0:
            solved_in_g2 += 1
            checks.append([(s, q)] * 3 + [(s, q_m3[qi])])
            want.append(1)
        else:
            checks.append([(s, q)] * 3 + [(CO.mul(s, R - 3), q)])
            want.append(1)
    assert want.count(0) >= 10 and solved_in_g2 >= 3
    t0 = time.perf_counter()
    got = _check_launch(eng, dev, checks)
    print("\npz_pairing_check_dev: 65 checks of 4 pairs %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    assert got == want
