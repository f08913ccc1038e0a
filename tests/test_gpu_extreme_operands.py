"""GPU: the scalar-field (Fr) kernels against the oracle on EXTREME and STRUCTURED operands (tests/extreme_operands.py).

The Fr kernels run on the 9 x 29-bit lazy representation of csrc/fp29.cuh, whose column accumulators have no carry-out; each carries a
hand-made bound analysis in its comments, and an operand past its analysed bound wraps silently.  Every other whole-kernel test feeds
uniformly random field elements: limbs uniform (a sum of k limbs sits near half its worst case), no stored word near r - 1, and no
intermediate ever EXACTLY zero -- so the canonicalisations on the way out (f29_canon_q, f29_to_fp<5>, f29_store_product, f29_is_zero) never
meet a k * p that must become 0 and not p.  Here the stored words have full limbs (2^253 - 1: eight full limbs, and f29_unpack_shl5's 32 x
image is full as well), are the largest legal ones (r - 1, r - 2), and the columns are constant / alternating / one-hot / geometric, whose
transforms, evaluations and quotients are exact zeros almost everywhere.

Every comparison is exact equality of the STORED WORDS against oracle/pyref.py or oracle/cref.py, or against a closed form in Python integers:
an oracle's values are turned into the canonical words the device must have written (_words), never the device's words into values -- a
stored p for 0, or x + p for x, is a mismatch.  The linear kernels' closed forms are stated in WORD space (word(a c) = word(a) c mod r,
tests/test_extreme_operands.py pins it).

What is exercised, per kernel ("classes": the 7 stored-word and 6 value classes; "challenges": the 12 challenge classes):
  ntt_dev forward + inverse with 1/n    log_n 1, 6, 9, 10, 11, 18, 19; constant column of every class (stored-word classes at 18, 19), one-hot at
                                        0 and n - 1, geometric, three alternating pairs, sprinkled
  ntt_dev coset pre-scale, post-scale   the same log_n; one-hot, constant r - 1 / 2^253 - 1, sprinkled; (g, s) over the challenges
  ntt_fr_to_dev                         the same log_n and patterns, strided input, omega^-1 and 1/n
  ntt_extend_dev, ntt_coeff_extend_dev  (log_n, log_e) (3,2) (9,2) (10,2) (11,1) (17,2); ten patterns; coset generator over the challenges
  poly_eval_dev, poly_eval_multi_dev    n 1, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8193; constant stored-word classes and alternating
                                        pairs; points 1, -1, 0, 2, 1/2, four word-space extremes, random; 1 to 4 points; planted roots
  poly_div_linear_dev                   n 1, 63, 64, 65, 16383, 16385; x 0, 1, -1, four word-space extremes; constant classes, one-hot; both ways
  fr_lincomb, fr_distribute_powers,     n 255, 256, 257; constant maximal, alternating, class walk, sprinkled; every scalar over the challenges
  fr_mul_row
  quotient_finish_dev                   (3,2) (6,1) (7,2); the same columns; coset generator over the challenges without +-1 (zero divisor)
  shplonk_begin / _finish               k = 5, 7 polynomials in 4 sets; y, v, u over the challenges; opening point a word extreme
  fr_batch_invert_dev                   n 1, 15, 16, 17, 4096, 4097 all-(r - 1), all-(2^253 - 1), classes mixed with zeros; 2^18 + 3, 2^19 + 3,
                                        2^20 + 3 sprinkled with zeros (chunk lengths 16, 32, 64)
  fr_prefix_product_dev                 the same small n; all-maximal and a late zero; z0 over the challenges
  permutation_product(_sets)_dev        log_n 4, 6; m 1, 3 and (5, 2); cells mixed classes, all 2^253 - 1, all r - 1; 24 (beta, gamma, z0) triples
  lookup_product_dev                    rows 50, 1000; four lookups of class columns; the same triples
  quotient_gate_dev                     (3,2,1) (5,2,3); each array maximal in turn, all at once, alternating runs, sprinkled, corners
  quotient_permutation_dev/_part/_split (m, chunk) (5,2) (7,3) (2,2) at k = 6; the same fills; beta, gamma, y, coset generator walked
  quotient_lookup_dev/_split, d_rows    three lookups, the same shapes and fills
  instance_eval_dev                     L 1, 64, 65; value classes; x word extremes and 1/2 (values), domain points (flag only)

What inputs cannot force: after the first product of a chain the limbs are pseudo-random whatever the input, so the LIMB bounds of later stages
(e.g. "limbs < 2^31.3" between the transform's stages, pz_ntt.hip) are reached by the first-stage operands only; for the later stages these
tests add the value-level cases: exact zeros, all-equal and sign-alternating operands, and the largest canonical words."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import extreme_operands as X
from tests import public_ref as PR

pytestmark = pytest.mark.gpu

R = X.R
DELTA = pow(P.FR_GENERATOR, 1 << P.FR_S, R)
CH = list(X.CHALLENGES.items())
STORED = list(X.WORD_CLASSES.items())
EVERY = list(X.ALL_WORDS.items())


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()  # torch fills / copies and the library's kernels in one order
    yield e
    e.close()


def _t(arr):
    """(.., 4) uint64 words -> int64 CUDA tensor"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).cuda()


def _tw(cols):
    """list of columns (lists of stored words) -> (ncols, n, 4) tensor; a single column -> (n, 4)"""
    if cols and isinstance(cols[0], (list, tuple)):
        return _t(np.stack([X.words_to_u64(c) for c in cols]))
    return _t(X.words_to_u64(cols))


def _u(t):
    return t.cpu().numpy().view(np.uint64)


def _w(t):
    """tensor -> flat list of stored words"""
    return X.u64_to_words(_u(t).reshape(-1, 4))


def F(value):
    """a challenge / constant VALUE -> the host array of its Montgomery word"""
    return X.word_u64(X.word_of(value))


def _vals(words):
    return [X.value_of(w) for w in words]


def _words(values):
    """oracle VALUES -> the canonical stored words the device must have written (a stored p for 0, or x + p for x, is a mismatch)"""
    return [X.word_of(v) for v in values]


def _chal(case, count):
    """the challenges of case number `case`, one per role: role k takes class (case + 5 k) mod 12, so that over any 12 consecutive cases every
    role meets every challenge class (names for the assertion messages, values)"""
    picks = [CH[(case + 5 * k) % len(CH)] for k in range(count)]
    return [nm for nm, _ in picks], [v for _, v in picks]


# ====================================================================================================================== transforms
NTT_LOGS = [1, 6, 9, 10, 11, 18, 19]   # one stage; small / largest single pass; smallest two-pass; odd first pass + lone radix-2; largest two-pass; three-pass


def _ntt_patterns(log_n):
    """(id, kind, payload) of the structured inputs; the value classes join the stored-word classes below 2^18"""
    classes = EVERY if log_n < 18 else STORED
    out = [("const:" + k, "const", w) for k, w in classes]
    for k in X.MAXIMAL:
        out += [("onehot0:" + k, "onehot", (0, X.ALL_WORDS[k])), ("onehotlast:" + k, "onehot", (-1, X.ALL_WORDS[k])),
                ("geom:" + k, "geom", X.ALL_WORDS[k])]
    out += [("alt:" + k, "alt", ab) for k, ab in X.ALT_PAIRS.items()]
    out.append(("sprinkled", "sprinkled", None))
    return out


NTT_CASES = [(l, pid, kind, pay) for l in NTT_LOGS for pid, kind, pay in _ntt_patterns(l)]


def _sparse(n, entries):
    a = np.zeros((n, 4), dtype=np.uint64)
    for i, w in entries.items():
        a[i] = X.word_u64(w % R)
    return a


def _ntt_input_and_want(cref, log_n, kind, pay, omega):
    """input (n, 4) words and the closed form of sum_j a[j] omega^(j k) (the oracle for the sprinkled column only)"""
    n = 1 << log_n
    if kind == "const":      # n a at index 0, EXACT zeros elsewhere
        return np.tile(X.word_u64(pay), (n, 1)), _sparse(n, {0: n * pay})
    if kind == "onehot":     # a geometric sequence: w omega^(p k)
        p, w = pay[0] % n, pay[1]
        return _sparse(n, {p: w}), X.words_to_u64(X.geometric(n, w, pow(omega, p, R)))
    if kind == "geom":       # c omega^(-j i): the single non-zero output n c at j
        j = (3 * n // 4 + 1) % n
        return X.words_to_u64(X.geometric(n, pay, pow(omega, -j, R))), _sparse(n, {j: n * pay})
    if kind == "alt":        # (a + b)/2 + (a - b)/2 (-1)^i: n (a + b)/2 at 0 and n (a - b)/2 at n/2
        a, b = pay
        return np.tile(X.words_to_u64([a, b]), (n // 2, 1)), _sparse(n, {0: (n // 2) * (a + b), n // 2: (n // 2) * (a - b)})
    x = X.sprinkled_u64(n, 1900 + log_n)
    return x, cref.ntt_fr(x, F(omega), log_n)


@pytest.mark.parametrize("log_n,pid,kind,pay", NTT_CASES, ids=["%d-%s" % (c[0], c[1]) for c in NTT_CASES])
def test_ntt_dev_forward_and_inverse(eng, cref, log_n, pid, kind, pay):
    """pz_ntt.hip "Tile elements stay UNCARRIED between stages (limbs < 2^31.3 ...) -- below 46p after 9 stages ... (14p in the first pair,
    whose operands come straight from the load)" and its two ways out, the product (ntt_store) and "canonical through the quotient estimate"
    (ntt_store_q / f29_canon_q, log_n = 1, 6, 9: single pass without a product).  A constant 2^253 - 1 column makes every first-stage operand
    of the load have full limbs, r - 1 the largest value; the constant, alternating and geometric columns put an exact 0 = k p in all but one
    or two outputs of the LAST stage, which must be stored as the zero word.  The inverse with the 1/n scale (the product way out) must return
    the input word for word."""
    n = 1 << log_n
    omega = P.fr_omega(log_n)
    x, want = _ntt_input_and_want(cref, log_n, kind, pay, omega)
    d = _t(x)
    eng.ntt_dev(d.data_ptr(), 1, 4 * n, F(omega), log_n)
    eng.sync()
    got = _u(d)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, ("forward", pid, "rows differing", bad.size, "first", int(bad[0]), X.u64_to_words(got[bad[:1]]), X.u64_to_words(want[bad[:1]]))
    eng.ntt_dev(d.data_ptr(), 1, 4 * n, F(pow(omega, -1, R)), log_n, None, F(pow(n, -1, R)))
    eng.sync()
    bad = np.nonzero((_u(d) != x).any(axis=1))[0]
    assert bad.size == 0, ("inverse", pid, "rows differing", bad.size, "first", int(bad[0]))


def _coset_pairs(log_n):
    """(coset generator, post scale) pairs: every challenge class in both roles below 2^18, the word-space extremes and -1 at size"""
    names = [k for k, _ in CH]
    pairs = [(names[i], names[(i + 3) % len(names)]) for i in range(len(names))]
    corners = [("c:2^253-1", "c:2^253-1"), ("c:r-1", "c:r-1")]     # both constants with extreme words at once
    return pairs + corners if log_n < 18 else [p for p in pairs if p[0] in ("c:2^253-1", "c:r-1", "c261:2^253-1", "v-1")] + corners


COSET_CASES = [(l, g, s) for l in NTT_LOGS for g, s in _coset_pairs(l)]


@pytest.mark.parametrize("log_n,gname,sname", COSET_CASES, ids=["%d-g=%s-s=%s" % c for c in COSET_CASES])
def test_ntt_dev_coset_pre_and_post_scale(eng, cref, log_n, gname, sname):
    """pz_ntt.hip "EVERY product of a transform is by a constant known in advance (twiddle, coset power, scale) ... f29_mulc takes 2^31.8 x 2^29
    limbs": the constants g^i and s come from the challenge classes, the ones whose Montgomery WORD is 2^253 - 1 or r - 1 included (constant
    operand with full limbs), g = 0, 1, -1 included (power tables 1 0 0 .., all ones, alternating sign).  out[k] = s sum_j a[j] g^j omega^(j k):
    one-hot columns in closed form (s w g^p omega^(p k)), the constant maximal and the sprinkled ones against oracle/cref.py."""
    n = 1 << log_n
    omega, g, s = P.fr_omega(log_n), X.CHALLENGES[gname], X.CHALLENGES[sname]
    wa, wb = X.ALL_WORDS["r-1"], X.ALL_WORDS["2^253-1"]
    cols = {"onehot0:r-1": _sparse(n, {0: wa}), "onehotlast:2^253-1": _sparse(n, {n - 1: wb}),
            "const:2^253-1": np.tile(X.word_u64(wb), (n, 1)), "const:r-1": np.tile(X.word_u64(wa), (n, 1)),
            "sprinkled": X.sprinkled_u64(n, 2900 + log_n)}
    names = list(cols)
    x = np.stack([cols[k] for k in names])
    d = _t(x)
    eng.ntt_dev(d.data_ptr(), len(names), 4 * n, F(omega), log_n, F(g), F(s))
    eng.sync()
    got = _u(d)
    for j, name in enumerate(names):
        want = cref.fr_scale(cref.ntt_fr(cref.fr_distribute_powers(x[j], F(g)), F(omega), log_n), F(s))
        assert np.array_equal(got[j], want), (name, "oracle")
    assert np.array_equal(got[0], X.words_to_u64([s * wa % R] * n))
    assert np.array_equal(got[1], X.words_to_u64(X.geometric(n, s * wb * pow(g, n - 1, R), pow(omega, n - 1, R))))


TO_DEV_CASES = [(l, grp) for l in NTT_LOGS for grp in ("constants", "structured", "sprinkled")]


@pytest.mark.parametrize("log_n,group", TO_DEV_CASES, ids=["%d-%s" % c for c in TO_DEV_CASES])
def test_ntt_fr_to_dev_out_of_place(eng, cref, log_n, group):
    """pz_ntt_fr_to_dev as lagrange_to_coeff calls it (omega^-1, post scale 1/n, strided input left untouched): the same first-stage operands
    (pz_ntt.hip "14p in the first pair, whose operands come straight from the load") through the out-of-place load path.  Constant Lagrange
    columns become the coefficient a and n - 1 exact zero words; one-hot, geometric and alternating columns in closed form."""
    n = 1 << log_n
    omega = P.fr_omega(log_n)
    w_inv, n_inv = pow(omega, -1, R), pow(n, -1, R)
    pats = [p for p in _ntt_patterns(log_n) if {"constants": p[1] == "const", "structured": p[1] in ("onehot", "geom", "alt"),
                                                "sprinkled": p[1] == "sprinkled"}[group]]
    ins, wants = zip(*[_ntt_input_and_want(cref, log_n, kind, pay, w_inv) for _, kind, pay in pats])
    x = np.zeros((len(pats), n + 8, 4), dtype=np.uint64)
    x[:, :n] = np.stack(ins)
    x[:, n:] = X.word_u64(R - 1)                 # the padding between strided columns must not be read
    d_in = _t(x)
    d_out = _t(np.zeros((len(pats), n, 4), dtype=np.uint64))
    eng.ntt_to_dev(d_in.data_ptr(), 4 * (n + 8), d_out.data_ptr(), 4 * n, len(pats), F(w_inv), log_n, None, F(n_inv))
    eng.sync()
    assert np.array_equal(_u(d_in), x)
    got = _u(d_out)
    for j, (pid, _, _) in enumerate(pats):
        want = cref.fr_scale(wants[j], F(n_inv))
        bad = np.nonzero((got[j] != want).any(axis=1))[0]
        assert bad.size == 0, (pid, "rows differing", bad.size, "first", int(bad[0]))


EXT_SHAPES = [(3, 2), (9, 2), (10, 2), (11, 1), (17, 2)]    # (17, 2): the at-scale arm of the four-coset layout
EXT_PATTERNS = ["const:r-1", "const:2^253-1", "const:w1", "const:top", "alt:w0|r-1", "alt:2^253-1|w0", "onehot0:r-1", "onehotlast:2^253-1",
                "geom:r-1", "sprinkled"]
EXT_CASES = [(s, p, CH[(i + 2 * j) % len(CH)][0]) for j, s in enumerate(EXT_SHAPES) for i, p in enumerate(EXT_PATTERNS)]


def _ext_column(n, pattern, log_n):
    kind, _, cls = pattern.partition(":")
    if kind == "const":
        return np.tile(X.word_u64(X.ALL_WORDS[cls]), (n, 1))
    if kind == "alt":
        return np.tile(X.words_to_u64(list(X.ALT_PAIRS[cls])), (n // 2, 1))
    if kind == "onehot0":
        return _sparse(n, {0: X.ALL_WORDS[cls]})
    if kind == "onehotlast":
        return _sparse(n, {n - 1: X.ALL_WORDS[cls]})
    if kind == "geom":
        return X.words_to_u64(X.geometric(n, X.ALL_WORDS[cls], pow(P.fr_omega(log_n), 5, R)))
    return X.sprinkled_u64(n, 3900 + log_n)


def _ext_oracle(cref, coeff, log_n, log_e, g):
    n, E = 1 << log_n, 1 << log_e
    ext = np.zeros((n * E, 4), dtype=np.uint64)
    ext[:n] = coeff
    return cref.ntt_fr(cref.fr_distribute_powers(ext, F(g)), F(P.fr_omega(log_n + log_e)), log_n + log_e)


@pytest.mark.parametrize("shape,pattern,gname", EXT_CASES, ids=["%d.%d-%s-g=%s" % (c[0][0], c[0][1], c[1], c[2]) for c in EXT_CASES])
def test_ntt_extend_and_coeff_extend(eng, cref, shape, pattern, gname):
    """pz_ntt.hip, the extended transforms: "A pass ends in a product wherever the algorithm has one (inter-pass twiddle, post scale: below 3p)
    and in the quotient-estimate canonicalisation (values below 64p) otherwise" -- coefficient columns with full limbs (2^253 - 1) and the
    largest words (r - 1) under coset generators from the challenge classes (g = 0: every coset power but the first is 0; g = 1: the constant
    column is n a at index 0 and an exact zero at every other multiple of 2^log_e; the word-space extremes: constant operands with full limbs).
    pz_ntt_fr_extend_dev against the oracle's zero-extend + distribute_powers + transform (and the one-hot closed form w g^p omega_ext^(p k));
    pz_ntt_fr_coeff_extend_dev from the Lagrange side: its coefficients against the oracle's inverse transform (a constant column: a and n - 1
    exact zeros, and then EVERY extended value equals a), its extended values against the oracle."""
    log_n, log_e = shape
    n, E = 1 << log_n, 1 << log_e
    g = X.CHALLENGES[gname]
    w_ext = P.fr_omega(log_n + log_e)
    w_n = pow(w_ext, E, R)
    gens = np.stack([F(g * pow(w_ext, r, R)) for r in range(E)])
    col = _ext_column(n, pattern, log_n)
    stride = 4 * n + 8
    d_c = _t(np.concatenate([col, np.tile(X.word_u64(R - 1), (2, 1))]))
    d_e = _t(np.zeros((n * E, 4), dtype=np.uint64))
    eng.ntt_extend_dev(d_c.data_ptr(), 1, stride, d_e.data_ptr(), 4 * n * E, log_n, log_e, F(w_n), gens, None)
    eng.sync()
    got = _u(d_e)
    assert np.array_equal(got, _ext_oracle(cref, col, log_n, log_e, g)), "extend"
    if pattern.startswith("onehot"):
        p, w = (0, X.ALL_WORDS["r-1"]) if pattern.startswith("onehot0") else (n - 1, X.ALL_WORDS["2^253-1"])
        assert np.array_equal(got, X.words_to_u64(X.geometric(n * E, w * pow(g, p, R), pow(w_ext, p, R)))), "extend, closed form"
    if pattern.startswith("const") and g == 1:
        assert X.u64_to_words(got[:1]) == [n * X.ALL_WORDS[pattern[6:]] % R] and not got[E::E].any()
    # the same column as LAGRANGE values
    d_v = _t(np.concatenate([col, np.tile(X.word_u64(R - 1), (2, 1))]))
    d_e2 = _t(np.zeros((n * E, 4), dtype=np.uint64))
    eng.ntt_coeff_extend_dev(d_v.data_ptr(), 1, stride, d_e2.data_ptr(), 4 * n * E, log_n, log_e, F(w_n), F(pow(w_n, -1, R)), F(pow(n, -1, R)), gens)
    eng.sync()
    coeff = cref.fr_scale(cref.ntt_fr(col, F(pow(w_n, -1, R)), log_n), F(pow(n, -1, R)))
    got_c, got_e = _u(d_v), _u(d_e2)
    assert np.array_equal(got_c[:n], coeff), "coefficients"
    assert X.u64_to_words(got_c[n:]) == [R - 1] * 2                              # the stride padding is not written
    assert np.array_equal(got_e, _ext_oracle(cref, coeff, log_n, log_e, g)), "coeff_extend"
    if pattern.startswith("const"):
        a = X.ALL_WORDS[pattern[6:]]
        assert X.u64_to_words(got_c[:1]) == [a] and not got_c[1:n].any()
        assert np.array_equal(got_e, np.tile(X.word_u64(a), (n * E, 1)))


# ====================================================================================================================== evaluation
EVAL_NS = [1, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8193]   # the 256-thread stride, the group of four terms, the 4096-coefficient block (1 and 2 partials)
EVAL_POINTS = [("v1", 1), ("v-1", R - 1), ("v0", 0), ("c:2^253-1", X.CHALLENGES["c:2^253-1"]), ("c:r-1", X.CHALLENGES["c:r-1"]),
               ("c261:2^253-1", X.CHALLENGES["c261:2^253-1"]), ("c261:r-1", X.CHALLENGES["c261:r-1"]), ("v2", 2), ("v(r+1)/2", (R + 1) // 2), ("random", random.Random(0xE7A1).randrange(R))]
_EVAL_COLS = {}


def _eval_columns(n):
    """the constant stored-word classes and the alternating pairs, as coefficient columns (built once per n)"""
    if n not in _EVAL_COLS:
        names = ["const:" + k for k, _ in STORED] + ["alt:" + k for k in X.ALT_PAIRS]
        cols = [X.constant(n, w) for _, w in STORED] + [X.alternating(n, a, b) for a, b in X.ALT_PAIRS.values()]
        _EVAL_COLS[n] = (names, cols)
    return _EVAL_COLS[n]


@pytest.mark.parametrize("pname,x", EVAL_POINTS, ids=[p[0] for p in EVAL_POINTS])
@pytest.mark.parametrize("n", EVAL_NS)
def test_poly_eval_extreme_points_and_columns(eng, n, pname, x):
    """pz_poly.hip k_poly_eval_partial_multi "Four terms share ONE Montgomery reduction (f29_dot4 ...); the EVAL_CH / 4 results are added
    limb-wise (limbs < 4 * 2^29, values < 8p)" and f29_to_fp<5> on the way out: the points 1, -1 and 0 give all-equal, sign-alternating and
    one-entry power tables, so with a constant r - 1 or 2^253 - 1 column f29_dot4 sums FOUR EQUAL MAXIMAL products (full limbs on the
    coefficient side; the table side is a product's output, pseudo-random except for those three points); the alternating columns at -1 and the
    constant ones at -1 (even n) sum to an exact zero."""
    names, cols = _eval_columns(n)
    d = _tw(cols)
    d_out = _t(np.zeros((len(cols), 4), dtype=np.uint64))
    eng.poly_eval_dev(d.data_ptr(), len(cols), 4 * n, n, F(x), d_out.data_ptr())
    eng.sync()
    got = _w(d_out)
    for j, name in enumerate(names):
        assert got[j] == P.poly_eval(cols[j], x), (name, pname)


MULTI_SETS = {1: ["c:r-1"], 2: ["v1", "v-1"], 3: ["v0", "c:2^253-1", "random"], 4: ["v-1", "c261:2^253-1", "c261:r-1", "v(r+1)/2"]}


@pytest.mark.parametrize("npts", [1, 2, 3, 4])
@pytest.mark.parametrize("n", EVAL_NS)
def test_poly_eval_multi_extreme_points_and_columns(eng, n, npts):
    """pz_poly.hip "the coefficient is read ONCE and multiplied into P accumulators": the same operands as the single-point test through the
    P = 1 .. 4 instantiations (each its own unrolled f29_dot4 chain and f29_to_fp<5> store)"""
    names, cols = _eval_columns(n)
    pts = [dict(EVAL_POINTS)[k] for k in MULTI_SETS[npts]]
    d = _tw(cols)
    d_out = _t(np.zeros((len(cols), npts, 4), dtype=np.uint64))
    eng.poly_eval_multi_dev(d.data_ptr(), len(cols), 4 * n, n, np.stack([F(x) for x in pts]), d_out.data_ptr())
    eng.sync()
    got = _w(d_out)
    for j, name in enumerate(names):
        for q, x in enumerate(pts):
            assert got[j * npts + q] == P.poly_eval(cols[j], x), (name, MULTI_SETS[npts][q])


@pytest.mark.parametrize("xname", ["v1", "v-1", "v2", "c:2^253-1", "c:r-1", "c261:2^253-1", "random"])
@pytest.mark.parametrize("n", EVAL_NS[1:])
def test_poly_eval_planted_root_is_the_zero_word(eng, n, xname):
    """pz_poly.hip: the partial sums leave through f29_to_fp<5> ("values < 8p") and are folded with fp_add; the coefficients of (t - x) q(t)
    evaluated at x sum to an exact 0 = k p, which must come out as the ZERO WORD, never as p (random coefficients never sum to zero)"""
    x = dict(EVAL_POINTS)[xname]
    q = X.sprinkled(n - 1, 4200 + n)
    c = [(-x * q[0]) % R] + [(q[i - 1] - x * q[i]) % R for i in range(1, n - 1)] + [q[n - 2]]
    assert len(c) == n and P.poly_eval(c, x) == 0
    others = [3, R - 1 if x != R - 1 else 1]
    d = _tw(c)
    d_out = _t(np.full((4, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    eng.poly_eval_dev(d.data_ptr(), 1, 4 * n, n, F(x), d_out[0].data_ptr())
    eng.poly_eval_multi_dev(d.data_ptr(), 1, 4 * n, n, np.stack([F(v) for v in [x] + others]), d_out[1].data_ptr())
    eng.sync()
    assert _w(d_out) == [0, 0] + [P.poly_eval(c, v) for v in others]


# ====================================================================================================================== division, fold, scaling
DIV_NS = [1, 63, 64, 65, 16383, 16385]      # 64: the chunk length; 16384: where a thread of the carry scan starts to own more than one chunk
DIV_POINTS = ["v0", "v1", "v-1", "c:2^253-1", "c:r-1", "c261:2^253-1", "c261:r-1"]


@pytest.mark.parametrize("xname", DIV_POINTS)
@pytest.mark.parametrize("n", DIV_NS)
def test_poly_div_linear_extreme(eng, n, xname):
    """pz_poly.hip kate division (chunks of 64 coefficients, carries x^64-scanned across chunks): x = 0 (the quotient is a shift: every carry
    is an exact zero), x = 1 (suffix sums: n equal maximal words accumulate), x = -1 (alternating suffix sums: a constant column's carries are
    0 or a, exactly), and the points whose Montgomery WORD is 2^253 - 1 / r - 1 (the power constants' limbs full); constant columns of every
    class and one-hot columns at 0, n - 1 and the chunk boundary, out of place and in place."""
    x = X.CHALLENGES[xname]
    cols = [X.constant(n, w) for _, w in EVERY]
    names = ["const:" + k for k, _ in EVERY]
    for k in X.MAXIMAL:
        for idx in sorted({0, n - 1, min(64, n - 1)}):
            cols.append(X.one_hot(n, idx, X.ALL_WORDS[k]))
            names.append("onehot%d:%s" % (idx, k))
    want = [P.kate_division(c, x) for c in cols]
    d = _tw(cols)
    d_q = _t(np.full((len(cols), n, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    eng.poly_div_linear_dev(d.data_ptr(), len(cols), 4 * n, n, F(x), d_q.data_ptr(), 4 * n)
    eng.sync()
    got = _w(d_q)
    for j, name in enumerate(names):
        assert got[j * n:(j + 1) * n] == want[j], (name, "out of place")
    eng.poly_div_linear_dev(d.data_ptr(), len(cols), 4 * n, n, F(x), d.data_ptr(), 4 * n)
    eng.sync()
    got = _w(d)
    for j, name in enumerate(names):
        assert got[j * n:(j + 1) * n] == want[j], (name, "in place")


BLOCK_NS = [255, 256, 257]                  # across one 256-thread block


def _class_columns(n, seed):
    """named columns of stored words for the element-wise kernels: the constant maximal classes, an alternating pair, a walk through every
    class, the sprinkled pattern"""
    ws = [w for _, w in EVERY]
    return {"const:r-1": X.constant(n, R - 1), "const:2^253-1": X.constant(n, (1 << 253) - 1), "alt:r-1|2^253-1": X.alternating(n, R - 1, (1 << 253) - 1),
            "walk": [ws[i % len(ws)] for i in range(n)], "sprinkled": X.sprinkled(n, seed)}


@pytest.mark.parametrize("vname", [k for k, _ in CH])
@pytest.mark.parametrize("n", BLOCK_NS)
def test_fr_lincomb_extreme(eng, n, vname):
    """pz_poly.hip pz_fr_lincomb_dev (acc = acc v + p_j over the columns, continued across calls): maximal words in every column with v from the
    challenge classes -- v = 0 keeps the last column only, v = -1 makes equal columns cancel to an exact zero word, the word-space extremes put
    full limbs on the constant side of every product; plain integer arithmetic is the reference"""
    v = X.CHALLENGES[vname]
    cols = list(_class_columns(n, 5100 + n).values())
    cols += [cols[0], cols[0]]                       # equal maximal columns: cancel under v = -1
    d = _tw(cols)
    d_o = _t(np.full((n, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    eng.fr_lincomb_dev(d.data_ptr(), 3, 4 * n, n, F(v), d_o.data_ptr())
    eng.fr_lincomb_dev(d[3].data_ptr(), len(cols) - 3, 4 * n, n, F(v), d_o.data_ptr(), True)
    eng.sync()
    want = [0] * n
    for c in cols:
        want = [(a * v + b) % R for a, b in zip(want, c)]
    assert _w(d_o) == want
    eng.fr_lincomb_dev(d[5].data_ptr(), 2, 4 * n, n, F(v), d_o.data_ptr())      # the two equal columns alone: a (v + 1)
    eng.sync()
    assert _w(d_o) == [a * (v + 1) % R for a in cols[0]]


PAIRS8 = [(CH[i][0], CH[(i + 5) % len(CH)][0]) for i in range(len(CH))]


@pytest.mark.parametrize("gname,cname", PAIRS8, ids=["g=%s-c=%s" % p for p in PAIRS8])
@pytest.mark.parametrize("n", BLOCK_NS)
def test_fr_distribute_powers_extreme(eng, n, gname, cname):
    """pz_poly.hip pz_fr_distribute_powers_dev (a[i] *= c g^i through the cached power table): g and c from the challenge classes (g = 0: the
    table is 1 0 0 ..; g = -1; the word-space extremes), data with full limbs and the largest words; c = NULL (= 1) included"""
    g, c = X.CHALLENGES[gname], X.CHALLENGES[cname]
    cols = list(_class_columns(n, 5200 + n).values())
    d = _tw(cols)
    eng.fr_distribute_powers_dev(d.data_ptr(), len(cols), 4 * n, n, F(g), F(c))
    eng.sync()
    got = _w(d)
    for j, col in enumerate(cols):
        assert got[j * n:(j + 1) * n] == P.distribute_powers(col, g, c), j
    d = _tw(cols)
    eng.fr_distribute_powers_dev(d.data_ptr(), len(cols), 4 * n, n, F(g))        # c = NULL -> 1
    eng.sync()
    got = _w(d)
    for j, col in enumerate(cols):
        assert got[j * n:(j + 1) * n] == P.distribute_powers(col, g), j


@pytest.mark.parametrize("n", BLOCK_NS)
def test_fr_mul_row_extreme(eng, n):
    """pz_quotient.hip pz_fr_mul_row_dev: both factors of every product from the classes (f29_load x f29_load_shl5: the 32 x image of 2^253 - 1
    has full limbs as well), every column against every row; integers are the reference (word(a b) = word(a) value(b))"""
    cols = _class_columns(n, 5300 + n)
    for rname, row in cols.items():
        d, d_row = _tw(list(cols.values())), _tw(row)
        eng.fr_mul_row_dev(d.data_ptr(), len(cols), 4 * n, n, d_row.data_ptr(), d.data_ptr(), 4 * n)       # in place
        eng.sync()
        rv = _vals(row)
        assert _w(d) == [a * b % R for col in cols.values() for a, b in zip(col, rv)], rname


# coset_g with (coset_g omega_ext^i)^n = 1 is outside pz_quotient_finish_dev's contract (pz.h: "d_h[i] /= (coset_g * omega_ext^i)^(2^log_n) - 1":
# a division by zero, which the oracle refuses as well): that leaves out g = 1 and g = -1
FINISH_G = [k for k, v in CH if v not in (1, R - 1)]


@pytest.mark.parametrize("gname", FINISH_G)
@pytest.mark.parametrize("log_n,log_e", [(3, 2), (6, 1), (7, 2)])
def test_quotient_finish_extreme(eng, log_n, log_e, gname):
    """pz_quotient.hip pz_quotient_finish_dev (h[i] times the inverse of the vanishing polynomial's 2^log_e values): h from the classes, the
    coset generator from the challenge classes (g = 0: every divisor is -1)"""
    g = X.CHALLENGES[gname]
    N = 1 << (log_n + log_e)
    w_ext = P.fr_omega(log_n + log_e)
    for name, col in _class_columns(N, 5400 + N).items():
        d = _tw(col)
        eng.quotient_finish_dev(d.data_ptr(), log_n, log_e, F(g), F(w_ext))
        eng.sync()
        assert _w(d) == P.quotient_finish(col, log_n, log_e, g, w_ext), name


SH_CASES = [(CH[i][0], CH[(i + 1) % len(CH)][0], CH[(i + 2) % len(CH)][0], ("c:2^253-1", "c:r-1")[(i + 1) % 2]) for i in range(len(CH))]


@pytest.mark.parametrize("yname,vname,uname,xname", SH_CASES, ids=["y=%s-v=%s-u=%s-x=%s" % c for c in SH_CASES])
def test_shplonk_extreme(eng, yname, vname, uname, xname):
    """pz_shplonk.hip "four terms share one Montgomery reduction (f29_dot4) ... each term < 1.8p, tight; at most SH_FOLD_CHUNK / 4 = 8 of them":
    k = 5, polynomials that are constant maximal / alternating / sprinkled columns, y, v, u from the challenge classes (y = 0 and v = 0 keep the
    first polynomial / set only; y = 1 folds equal maximal columns with all-one powers), the opening point a word-space extreme; both output
    polynomials against P.shplonk_h2"""
    k = 5
    n = 1 << k
    w = P.fr_omega(k)
    y, v, u, x = (X.CHALLENGES[nm] for nm in (yname, vname, uname, xname))
    points = [x, x * w % R, x * pow(w, -1, R) % R, x * pow(w, n - 11, R) % R]
    assert len(set(points)) == 4 and u not in points
    base = list(_class_columns(n, 5500).values())
    polys = base + [X.constant(n, R - 2), X.alternating(n, 0, R - 1)]        # 7 polynomials of stored words
    groups = [([0, 1, 2], [0]), ([3, 4], [0, 1]), ([5], [0, 1, 2]), ([6], [0, 3])]
    vals = [_vals(p) for p in polys]
    d_p = _tw(polys)
    sets_dev, sets_ref = [], []
    for ids, idx in groups:
        ev = np.stack([np.stack([F(P.poly_eval(vals[i], points[t])) for t in idx]) for i in ids])
        sets_dev.append(([d_p[i].data_ptr() for i in ids], idx, ev))
        sets_ref.append(([vals[i] for i in ids], idx))
    d_h = _t(np.zeros((n, 4), dtype=np.uint64))
    d_h2 = _t(np.zeros((n, 4), dtype=np.uint64))
    st = eng.shplonk_begin_dev(n, sets_dev, np.stack([F(p) for p in points]), F(y), F(v), d_h.data_ptr())
    eng.sync()
    want_h, want_h2, _ = P.shplonk_h2(sets_ref, points, y, v, u, n)
    assert _w(d_h) == _words(want_h)
    eng.shplonk_finish_dev(st, F(u), d_h.data_ptr(), d_h2.data_ptr())
    eng.sync()
    assert _w(d_h2) == _words(want_h2)


# ====================================================================================================================== inversion and scans
SCAN_NS = [1, 15, 16, 17, 4096, 4097]


@pytest.mark.parametrize("cls", X.MAXIMAL)
@pytest.mark.parametrize("n", SCAN_NS)
def test_batch_invert_extreme(eng, n, cls):
    """pz_quotient.hip k_batch_invert ("acc is a product of non-zero elements (or 1)"; f29_from_fp_shl5 of the stored word; the inverse leaves
    through f29_store_product): all-(r - 1) and all-(2^253 - 1) words -- the 32 x image of every factor has full limbs, r - 1 is its own
    inverse so every running product is +-1 -- and the classes mixed with zeros, which stay zero"""
    w = X.ALL_WORDS[cls]
    inv = X.word_of(pow(X.value_of(w), -1, R))
    d = _tw(X.constant(n, w))
    eng.fr_batch_invert_dev(d.data_ptr(), n)
    eng.sync()
    assert _w(d) == [inv] * n
    ws = [w_ for _, w_ in EVERY]
    mixed = [0 if i % 3 == 1 else ws[(i // 3) % len(ws)] for i in range(n)]
    d = _tw(mixed)
    eng.fr_batch_invert_dev(d.data_ptr(), n)
    eng.sync()
    assert _w(d) == _words(P.batch_invert(_vals(mixed)))


@pytest.mark.parametrize("n", [(1 << 18) + 3, (1 << 19) + 3, (1 << 20) + 3])
def test_batch_invert_longer_chunks(eng, n):
    """pz_quotient.hip pz_batch_invert_internal picks its chunk length by size ("K = 64 once there are 2^14 threads, up to 512 while 2^18
    threads ... remain"): K = 8 below 2^18 elements, then 16, 32, 64 at these three sizes (K >= 128 needs n / 128 >= 2^18, that is 2^25 elements:
    1 GiB of data plus 1 GiB of scratch, and stays out of the suite).  Sprinkled data with zeros: every element satisfies a a^-1 == 1 (or is 0 where a is 0)
    in Python integers, and 200 sampled elements equal P.batch_invert."""
    x = X.sprinkled_u64(n, 6000 + n)
    x[::7] = 0
    d = _t(x)
    eng.fr_batch_invert_dev(d.data_ptr(), n)
    eng.sync()
    a, got = X.u64_to_words(x), _w(d)
    one = X.MONT * X.MONT % R            # word(a) word(1/a) = 2^512 mod r
    assert all(g < R for g in got)                                                # canonical words: g + r would pass the product check below
    assert all((g * w % R == one) if w else g == 0 for w, g in zip(a, got))
    idx = random.Random(n).sample(range(n), 200) + [0, 1, n - 1]
    assert [got[i] for i in idx] == _words(P.batch_invert(_vals([a[i] for i in idx])))


@pytest.mark.parametrize("zname", [k for k, _ in CH])
@pytest.mark.parametrize("n", SCAN_NS)
def test_prefix_product_extreme(eng, n, zname):
    """pz_quotient.hip k_pp_local / k_pp_apply ("the run product stays in the 256-domain through shl5-unpacked factors; the workgroup scan runs
    in the 261-domain ... `excl` keeps that domain -- packed, not canonical"; every z leaves through f29_store_product): all-(r - 1) words (the
    scan's operands are +-1: the largest and the smallest values), all-(2^253 - 1) words (full limbs in x and 32 x), classes mixed with zeros
    (every later product is an exact zero), z0 from the challenge classes; out of place and in place"""
    z0 = X.CHALLENGES[zname]
    ws = [w_ for _, w_ in EVERY]
    cols = {"all:r-1": X.constant(n, R - 1), "all:2^253-1": X.constant(n, (1 << 253) - 1),
            "zeros-late": [0 if i == (2 * n) // 3 else ws[i % len(ws)] or 1 for i in range(n)]}
    for name, col in cols.items():
        want = [X.word_of(v) for v in P.prefix_product(_vals(col), z0)]
        d = _tw(col)
        d_z = _t(np.full((n, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
        eng.fr_prefix_product_dev(d.data_ptr(), n, F(z0), d_z.data_ptr())
        eng.sync()
        assert _w(d_z) == want, name
        eng.fr_prefix_product_dev(d.data_ptr(), n, F(z0), d.data_ptr())
        eng.sync()
        assert _w(d) == want, (name, "in place")


# ====================================================================================================================== grand products
BG = [(CH[i][0], CH[(i + k) % len(CH)][0], CH[(i + 2 * k + 1) % len(CH)][0]) for k in (0, 3) for i in range(len(CH))]


CELLS = ["mixed", "2^253-1", "r-1"]


def _permutation_world(rng, n, m, rows, cell_class="mixed"):
    """a real permutation of the m * rows cells (identity on the rows above) with values constant on its cycles, the values drawn from the
    stored-word classes (as VALUES the oracle sees value_of(word)), or every cell the one maximal word `cell_class` names: the product still
    telescopes"""
    omega = P.fr_omega(n.bit_length() - 1)
    labels = [[pow(DELTA, j, R) * pow(omega, i, R) % R for i in range(n)] for j in range(m)]
    cells = [(j, i) for j in range(m) for i in range(rows)]
    perm = list(cells)
    rng.shuffle(perm)
    to = dict(zip(cells, perm))
    sigma = [list(l) for l in labels]
    words = [w for _, w in STORED] if cell_class == "mixed" else [X.ALL_WORDS[cell_class]]
    val = [[rng.choice(words) for _ in range(n)] for _ in range(m)]
    seen = set()
    for cell in cells:
        if cell in seen:
            continue
        w, cur = rng.choice(words), cell
        while cur not in seen:
            seen.add(cur)
            val[cur[0]][cur[1]] = w
            cur = to[cur]
    for (j, i), (pj, pi) in to.items():
        sigma[j][i] = labels[pj][pi]
    return omega, labels, val, sigma


@pytest.mark.parametrize("bname,gname,zname", BG, ids=["b=%s-g=%s-z0=%s" % c for c in BG])
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("log_n,m", [(4, 1), (6, 3)])
def test_permutation_product_extreme(eng, log_n, m, cells, bname, gname, zname):
    """pz_quotient.hip permutation product ("one256 (an empty set) or a product: strict limbs, below 2p", k_batch_invert's fused num / den and
    the scan): cell values from the stored-word classes on a real permutation's cycles, beta, gamma, z0 from the challenge classes, 0 included
    -- v + beta sigma + gamma sums up to three maximal tight values (every cell 2^253 - 1 with beta = gamma = the value whose word is 2^253 - 1 fills the
    limbs of the 32 x image of v and of gamma at once; sigma holds the permutation's labels and cannot be chosen), and ZERO DENOMINATORS arise by construction (beta = gamma = 0 on a zero
    cell; gamma = -v): the expected value is the oracle's, where the inverse of zero is zero"""
    n = 1 << log_n
    rng = random.Random(7000 + log_n)
    beta, gamma, z0 = (X.CHALLENGES[k] for k in (bname, gname, zname))
    omega, labels, val, sigma = _permutation_world(rng, n, m, n, cells)
    stride = 4 * n + 8
    d_cols = _t(np.zeros((m, n + 2, 4), dtype=np.uint64))
    d_sig = _t(np.zeros((m, n + 2, 4), dtype=np.uint64))
    d_cols[:, :n] = _tw(val)
    d_sig[:, :n] = _tw([[X.word_of(s) for s in col] for col in sigma])
    d_z = _t(np.zeros((n, 4), dtype=np.uint64))
    eng.permutation_product_dev(d_cols.data_ptr(), stride, d_sig.data_ptr(), stride, m, log_n, F(omega), F(beta), F(gamma), F(1), F(DELTA), F(z0),
                                d_z.data_ptr())
    eng.sync()
    vv = [_vals(c) for c in val]
    assert _w(d_z) == _words(P.permutation_product(vv, sigma, omega, beta, gamma, 1, DELTA, z0))


@pytest.mark.parametrize("bname,gname", [c[:2] for c in BG], ids=["b=%s-g=%s" % c[:2] for c in BG])
@pytest.mark.parametrize("cells", CELLS)
@pytest.mark.parametrize("log_n", [4, 6])
def test_permutation_product_sets_extreme(eng, log_n, cells, bname, gname):
    """pz_quotient.hip pz_permutation_product_sets_dev, (m, chunk) = (5, 2): the short last set ("one256 (an empty set) or a product"), the
    chaining z_j[0] = z_(j-1)[usable rows] -- the same extreme cells and challenges as the single-chunk test; set by set against
    P.permutation_product"""
    n, m, chunk = 1 << log_n, 5, 2
    u = n - 6
    rng = random.Random(7100 + log_n)
    beta, gamma = X.CHALLENGES[bname], X.CHALLENGES[gname]
    omega, labels, val, sigma = _permutation_world(rng, n, m, u, cells)
    nsets = -(-m // chunk)
    d_val, d_sig = _tw(val), _tw([[X.word_of(s) for s in col] for col in sigma])
    d_z = _t(np.zeros((nsets, n, 4), dtype=np.uint64))
    eng.permutation_product_sets_dev(d_val.data_ptr(), 4 * n, d_sig.data_ptr(), 4 * n, m, chunk, log_n, u, F(omega), F(beta), F(gamma), F(DELTA),
                                     d_z.data_ptr(), 4 * n)
    eng.sync()
    vv = [_vals(c) for c in val]
    z0 = 1
    for j in range(nsets):
        c0 = j * chunk
        want = P.permutation_product(vv[c0:c0 + chunk], sigma[c0:c0 + chunk], omega, beta, gamma, pow(DELTA, c0, R), DELTA, z0)
        got = _w(d_z[j])
        assert got == _words(want), ("set", j)
        z0 = want[u]


@pytest.mark.parametrize("bname,gname,zname", BG, ids=["b=%s-g=%s-z0=%s" % c for c in BG])
@pytest.mark.parametrize("rows", [50, 1000])
def test_lookup_product_extreme(eng, rows, bname, gname, zname):
    """pz_lookup.hip / pz_quotient.hip lookup product ((A + beta)(S + gamma) / ((A' + beta)(S' + gamma)) through the fused inversion and the
    batched scan): all four columns from the classes (constant maximal, alternating, a walk through every class, sprinkled), beta, gamma, z0
    from the challenge classes, 0 included; zero denominators arise by construction (beta = 0 on a zero cell, beta = 1 on r - 1 ...) and give
    the oracle's value, where the inverse of zero is zero"""
    beta, gamma, z0 = (X.CHALLENGES[k] for k in (bname, gname, zname))
    vals = lambda w: [X.word_of(v) for v in w]   # these classes are meant as VALUES here: the sums v + beta meet 0 and r exactly
    cols = list(_class_columns(rows, 7200 + rows).values())
    A, Ap, Sp = cols[0:3], cols[2:5], [cols[3], cols[0], cols[1]]
    S = cols[4]
    small = [vals([(i * 7) % 5 for i in range(rows)]), vals([R - 1 - (i % 3) for i in range(rows)])]
    A, Ap, Sp = A + [small[0]], Ap + [small[1]], Sp + [small[0]]
    nl = len(A)
    d_A, d_S, d_Ap, d_Sp = _tw(A), _tw(S), _tw(Ap), _tw(Sp)
    d_z = _t(np.zeros((nl, rows, 4), dtype=np.uint64))
    eng.lookup_product_dev(d_A.data_ptr(), 4 * rows, d_S.data_ptr(), d_Ap.data_ptr(), 4 * rows, d_Sp.data_ptr(), 4 * rows, nl, rows, F(beta), F(gamma),
                           F(z0), d_z.data_ptr(), 4 * rows)
    eng.sync()
    for j in range(nl):
        assert _w(d_z[j]) == _words(P.lookup_product(_vals(A[j]), _vals(S), _vals(Ap[j]), _vals(Sp[j]), beta, gamma, z0)), j


# ====================================================================================================================== quotient lines
CORNERS = [(d, pre + c) for d in X.MAXIMAL for pre in ("c:", "c261:", "c266:") for c in X.MAXIMAL]


def _fills(names):
    """(id, {array name: class}, forced challenge class or None): every input array in turn filled with a constant maximal class (the others sprinkled), all at once; the same
    with runs of two maximal words and two zeros ("alt:": a rotation by one domain row then meets the other value); the CORNERS -- every array
    one maximal class and every challenge the value whose Montgomery word, or whose 2^261 / 2^266 image (the limb form in the scalar registers:
    host_fr_shl), is a maximal class, the operands the analysed limb bounds speak of;
    and the sprinkled pattern everywhere, once per challenge class"""
    out = []
    for cls in X.MAXIMAL:
        for nm in names:
            out.append(("%s=%s" % (nm, cls), {nm: cls}, None))
        out.append(("all=%s" % cls, {nm: cls for nm in names}, None))
        out.append(("all=alt:%s" % cls, {nm: "alt:" + cls for nm in names}, None))
    out += [("%s=alt:2^253-1" % nm, {nm: "alt:2^253-1"}, None) for nm in names]
    out += [("sprinkled%d" % i, {}, None) for i in range(len(CH))]    # one per challenge class: each role meets every class here alone
    for d, c in CORNERS:
        out.append(("corner:data=%s,challenges=%s" % (d, c), {nm: d for nm in names}, c))
    return out


def _fill_chal(case, count, forced):
    """the case's challenges: the corner's forced class in every role, else the deterministic walk of _chal"""
    if forced is not None:
        return [forced] * count, [X.CHALLENGES[forced]] * count
    return _chal(case, count)


def _fill_column(length, cls):
    if cls.startswith("alt:"):
        w = X.ALL_WORDS[cls[4:]]
        return [w if (i // 2) % 2 == 0 else 0 for i in range(length)]
    return X.constant(length, X.ALL_WORDS[cls])


def _filled(rng_seed, fill, shapes):
    """name -> list of columns of stored words ((count, length) per name): the class `fill` names, sprinkled otherwise"""
    out = {}
    for i, (nm, (count, length)) in enumerate(shapes.items()):
        if nm in fill:
            out[nm] = [_fill_column(length, fill[nm]) for _ in range(count)]
        else:
            out[nm] = [X.sprinkled(length, rng_seed + 100 * i + c) for c in range(count)]
    return out


GATE_FILLS = _fills(["adv", "sel", "h"])
GATE_CASES = [(s, i) for s in [(3, 2, 1), (5, 2, 3)] for i in range(len(GATE_FILLS))]


@pytest.mark.parametrize("shape,fi", GATE_CASES, ids=["%d.%d.%d-%s" % (c[0] + (GATE_FILLS[c[1]][0],)) for c in GATE_CASES])
def test_quotient_gate_extreme(eng, shape, fi):
    """pz_quotient.hip gate line "e = a0 + a1 a2 - a3 + 2p: limbs < 2^31, value < 4.2p": advice constant r - 1 makes a0 maximal, a1 a2 = 1 and
    a3 maximal (e = 1 exactly), constant 2^253 - 1 fills every limb of the three loaded operands; selector and incoming h maximal in turn and
    all at once; y from the challenge classes (0 and the word-space extremes included).  Against P.quotient_gate."""
    log_n, log_e, ncols = shape
    fid, fill, forced = GATE_FILLS[fi]
    N, step = 1 << (log_n + log_e), 1 << log_e
    (yname,), (y,) = _fill_chal(fi, 1, forced)
    c = _filled(8100 + fi, fill, {"adv": (ncols, N), "sel": (ncols, N), "h": (1, N)})
    d_a, d_s, d_h = _tw(c["adv"]), _tw(c["sel"]), _tw(c["h"][0])
    eng.quotient_gate_dev(d_a.data_ptr(), 4 * N, d_s.data_ptr(), 4 * N, ncols, log_n + log_e, step, F(y), d_h.data_ptr())
    eng.sync()
    want = P.quotient_gate([_vals(x) for x in c["adv"]], [_vals(x) for x in c["sel"]], step, y, _vals(c["h"][0]))
    assert _w(d_h) == _words(want), (fid, yname)


K, BF = 6, 5
NK = 1 << K
U = NK - (BF + 1)
SHAPES = [(5, 2), (7, 3), (2, 2)]        # tests/test_gpu_two_coset_lines.py
LK = 3
PERM_FILLS = _fills(["cols", "sig", "z", "l0", "l_last", "l_active", "h"])
PERM_CASES = [(s, i) for s in SHAPES for i in range(len(PERM_FILLS))]


@pytest.mark.parametrize("shape,fi", PERM_CASES, ids=["%d.%d-%s" % (c[0] + (PERM_FILLS[c[1]][0],)) for c in PERM_CASES])
def test_quotient_permutation_lines_extreme(eng, shape, fi):
    """pz_quotient.hip permutation lines: "loose x loose limbs: 9 * 2^30 * 2^30 + 2^59.8 < 2^64; value < 8p" and the sums of up to three tight
    values v + beta sigma + gamma / f29_sub<2, 29> operands: every input array (columns, sigma, z, l0, l_last, l_active, incoming h) in turn a
    constant r - 1 (the largest value: 1 - z, z^2 - z and z_j - z_(j-1) are 2, 2 and an exact 0) or 2^253 - 1 (full limbs), all at once, and
    sprinkled; beta, gamma, y and the coset generator from the challenge classes.  pz_quotient_permutation_dev against
    P.quotient_permutation; the _part form in two set ranges gives the same words; the _split form's Low + l_active D sums to them."""
    m, chunk = shape
    fid, fill, forced = PERM_FILLS[fi]
    log_ext, rot = K + 1, 2
    Ne = 1 << log_ext
    S = -(-m // chunk)
    w_ext = P.fr_omega(log_ext)
    cnames, (beta, gamma, y, cg) = _fill_chal(fi, 4, forced)
    c = _filled(8300 + fi, fill, {"cols": (m, Ne), "sig": (m, Ne), "z": (S, Ne), "l0": (1, Ne), "l_last": (1, Ne), "l_active": (1, Ne), "h": (1, Ne)})
    V = {k: [_vals(x) for x in v] for k, v in c.items()}
    cols, sig, z = _tw(c["cols"]), _tw(c["sig"]), _tw(c["z"])
    l0, ll, la = _tw(c["l0"][0]), _tw(c["l_last"][0]), _tw(c["l_active"][0])
    chal = (F(beta), F(gamma), F(DELTA), F(cg), F(w_ext), F(y))
    want = P.quotient_permutation(V["cols"], V["sig"], V["z"], chunk, rot, BF + 1, V["l0"][0], V["l_last"][0], V["l_active"][0], beta, gamma, DELTA, cg,
                                  w_ext, y, V["h"][0])
    d_h = _tw(c["h"][0])
    eng.quotient_permutation_dev(cols.data_ptr(), 4 * Ne, sig.data_ptr(), 4 * Ne, z.data_ptr(), 4 * Ne, S, chunk, m, log_ext, rot, BF + 1,
                                 l0.data_ptr(), ll.data_ptr(), la.data_ptr(), *chal, d_h.data_ptr())
    eng.sync()
    assert _w(d_h) == _words(want), (fid, cnames, "unsplit")
    # set ranges: the part form, and the split form from h (Low) and 0 (D)
    d_hp, low, dd = _tw(c["h"][0]), _tw(c["h"][0]), _t(np.zeros((Ne, 4), dtype=np.uint64))
    ranges = [(0, 2), (2, 1)] if S == 3 else [(0, 1)]
    for set_lo, ns in ranges:
        c0 = set_lo * chunk
        cnt = min(m - c0, ns * chunk)
        common = (cols[c0].data_ptr(), 4 * Ne, sig[c0].data_ptr(), 4 * Ne, z.data_ptr(), 4 * Ne, S, set_lo, ns, chunk, cnt, set_lo == 0, log_ext, rot,
                  BF + 1, l0.data_ptr(), ll.data_ptr())
        eng.quotient_permutation_part_dev(*common, la.data_ptr(), *chal, d_hp.data_ptr())
        eng.quotient_permutation_split_dev(*common, *chal, low.data_ptr(), dd.data_ptr())
    eng.sync()
    assert _w(d_hp) == _words(want), (fid, cnames, "part")
    w_low, w_d = _w(low), _w(dd)
    assert all(w < R for w in w_low + w_d), (fid, cnames, "split: canonical words")
    assert [(lo + a * d) % R for lo, a, d in zip(w_low, V["l_active"][0], w_d)] == _words(want), (fid, cnames, "split")


LOOK_FILLS = _fills(["a", "table", "ap", "sp", "zl", "l0", "l_last", "l_active", "h"])


@pytest.mark.parametrize("fi", range(len(LOOK_FILLS)), ids=[f[0] for f in LOOK_FILLS])
def test_quotient_lookup_lines_extreme(eng, fi):
    """pz_quotient.hip lookup lines (the same "loose x loose" products and f29_sub<2, 29> operands; a' - s' and a' - a'(w^-1 X) are EXACT ZEROS
    on constant columns, z^2 - z is 2 at r - 1): every input array in turn a constant maximal class, all at once, and sprinkled; beta, gamma, y
    from the challenge classes.  pz_quotient_lookup_dev against P.quotient_lookup; the _split form sums to the same words."""
    fid, fill, forced = LOOK_FILLS[fi]
    log_ext, rot = K + 1, 2
    Ne = 1 << log_ext
    cnames, (beta, gamma, y) = _fill_chal(fi, 3, forced)
    c = _filled(8500 + fi, fill, {"a": (LK, Ne), "table": (1, Ne), "ap": (LK, Ne), "sp": (LK, Ne), "zl": (LK, Ne), "l0": (1, Ne), "l_last": (1, Ne),
                                  "l_active": (1, Ne), "h": (1, Ne)})
    V = {k: [_vals(x) for x in v] for k, v in c.items()}
    a, ap, sp, zl, table = _tw(c["a"]), _tw(c["ap"]), _tw(c["sp"]), _tw(c["zl"]), _tw(c["table"][0])
    l0, ll, la = _tw(c["l0"][0]), _tw(c["l_last"][0]), _tw(c["l_active"][0])
    lk = (a.data_ptr(), 4 * Ne, table.data_ptr(), ap.data_ptr(), 4 * Ne, sp.data_ptr(), 4 * Ne, zl.data_ptr(), 4 * Ne, LK, log_ext, rot, l0.data_ptr(),
          ll.data_ptr(), la.data_ptr(), F(beta), F(gamma), F(y))
    want = P.quotient_lookup(V["a"], V["table"][0], V["ap"], V["sp"], V["zl"], rot, V["l0"][0], V["l_last"][0], V["l_active"][0], beta, gamma, y,
                             V["h"][0])
    d_h, low, dd = _tw(c["h"][0]), _tw(c["h"][0]), _t(np.zeros((Ne, 4), dtype=np.uint64))
    eng.quotient_lookup_dev(*lk, d_h.data_ptr())
    eng.quotient_lookup_split_dev(*lk, low.data_ptr(), dd.data_ptr())
    eng.sync()
    assert _w(d_h) == _words(want), (fid, cnames, "unsplit")
    w_low, w_d = _w(low), _w(dd)
    assert all(w < R for w in w_low + w_d), (fid, cnames, "split: canonical words")
    assert [(lo + x * d) % R for lo, x, d in zip(w_low, V["l_active"][0], w_d)] == _words(want), (fid, cnames, "split")


DROW_FILLS = _fills(["cols", "sig", "z", "a", "table", "ap", "sp", "zl"])
DROW_CASES = [(s, i) for s in SHAPES for i in range(len(DROW_FILLS))]


def _roles_meet_every_class(fills, roles):
    """every challenge role of a line test meets every challenge class among the cases that do not force their challenges"""
    seen = [set() for _ in range(roles)]
    for fi, (_, _, forced) in enumerate(fills):
        if forced is None:
            for k, nm in enumerate(_chal(fi, roles)[0]):
                seen[k].add(nm)
    return all(sn == set(X.CHALLENGES) for sn in seen)


assert _roles_meet_every_class(GATE_FILLS, 1) and _roles_meet_every_class(PERM_FILLS, 4)
assert _roles_meet_every_class(LOOK_FILLS, 3) and _roles_meet_every_class(DROW_FILLS, 3)


@pytest.mark.parametrize("shape,fi", DROW_CASES, ids=["%d.%d-%s" % (c[0] + (DROW_FILLS[c[1]][0],)) for c in DROW_CASES])
def test_quotient_d_rows_extreme(eng, shape, fi):
    """pz_quotient.hip pz_quotient_d_rows_dev (the product lines' weighted sum on the last rows of the domain, from the Lagrange forms; the rows
    below row_lo WRITTEN as zero): every input array in turn a constant maximal class, all at once, and sprinkled; beta, gamma, y from the
    challenge classes; the wrap of row n - 1 to z(w^0) included.  Against the integer restatement of tests/test_gpu_two_coset_lines.py."""
    m, chunk = shape
    fid, fill, forced = DROW_FILLS[fi]
    S = -(-m // chunk)
    w = P.fr_omega(K)
    cnames, (beta, gamma, y) = _fill_chal(fi, 3, forced)
    c = _filled(8700 + fi, fill, {"cols": (m, NK), "sig": (m, NK), "z": (S, NK), "a": (LK, NK), "table": (1, NK), "ap": (LK, NK), "sp": (LK, NK),
                                  "zl": (LK, NK)})
    V = {k: [_vals(x) for x in v] for k, v in c.items()}
    cols, sig, z, a, ap, sp, zl = (V[k] for k in ("cols", "sig", "z", "a", "ap", "sp", "zl"))
    table = V["table"][0]
    want = [0] * NK
    for i in range(U, NK):
        nx = (i + 1) % NK                                 # row n - 1 reads z(w^0)
        acc = 0
        for j in range(S):
            left, right = z[j][nx], z[j][i]
            for cc in range(j * chunk, min(m, (j + 1) * chunk)):
                left = left * (cols[cc][i] + beta * sig[cc][i] + gamma) % R
                right = right * (cols[cc][i] + beta * pow(DELTA, cc, R) * pow(w, i, R) + gamma) % R
            acc += (left - right) * pow(y, (S - 1 - j) + 5 * LK, R)
        for l in range(LK):
            d = zl[l][nx] * (ap[l][i] + beta) * (sp[l][i] + gamma) - zl[l][i] * (a[l][i] + beta) * (table[i] + gamma)
            acc += d * pow(y, 5 * (LK - 1 - l) + 2, R)
        want[i] = acc % R
    d_ = {k: _tw(v) for k, v in c.items()}
    out = _t(np.full((NK, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    eng.quotient_d_rows_dev(d_["cols"].data_ptr(), 4 * NK, d_["sig"].data_ptr(), 4 * NK, d_["z"].data_ptr(), 4 * NK, m, chunk, d_["a"].data_ptr(), 4 * NK,
                            d_["table"].data_ptr(), d_["ap"].data_ptr(), 4 * NK, d_["sp"].data_ptr(), 4 * NK, d_["zl"].data_ptr(), 4 * NK, LK, K, U, F(w),
                            F(beta), F(gamma), F(DELTA), F(y), out.data_ptr())
    eng.sync()
    assert _w(out) == _words(want), (fid, cnames)


# ====================================================================================================================== public inputs
@pytest.mark.parametrize("L", [1, 64, 65])
def test_instance_eval_extreme(eng, L):
    """pz_public.hip k_instance_eval (the Lagrange-basis sum with one batched inversion per 1024 terms): instance values from the value classes
    (canonical words: 0, 1, 2, r - 1 and the two halves), x a word-space extreme.  A domain point is outside the value contract (pz.h: "bit 0
    x_p lies on the domain (a zero denominator, or x^n = 1) ... d_out[p] is then meaningless"): for those the FLAG is what is checked."""
    import torch

    k = 10
    classes = list(X.VALUE_CLASSES.values())
    w = P.fr_omega(k)
    xs = [X.CHALLENGES["c:2^253-1"], X.CHALLENGES["c:r-1"], pow(w, L - 1, R), 1, R - 1, (R + 1) // 2]
    B = len(xs)
    vals = [[classes[(i + b) % len(classes)] if b else R - 1 for i in range(L)] for b in range(B)]
    d_inst = _t(np.stack([X.words_to_u64(v) for v in vals]))                     # CANONICAL words
    d_x = _t(np.stack([F(x) for x in xs]))
    d_out = _t(np.zeros((B, 4), dtype=np.uint64))
    d_fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    om, ninv = F(w), F(pow(1 << k, -1, R))
    eng.sync()
    eng._chk(eng.L.pz_instance_eval_dev(eng.ctx, k, om.ctypes.data, ninv.ctypes.data, d_inst.data_ptr(), L, B, d_x.data_ptr(), d_out.data_ptr(),
                                        d_fl.data_ptr()), "pz_instance_eval_dev")
    eng.sync()
    got, flags = _w(d_out), d_fl.cpu().numpy().tolist()
    assert flags == [0, 0, 1, 1, 1, 0]
    for b in (0, 1, 5):
        assert got[b] == X.word_of(PR.instance_eval(k, vals[b], xs[b])), b
