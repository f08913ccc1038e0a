"""CPU: the operand classes of tests/extreme_operands.py are what they claim, and both oracles accept them.

The GPU tests (tests/test_gpu_extreme_operands.py) hold the Fr kernels to oracle/pyref.py and oracle/cref.py on these classes, so the classes'
limb patterns and the oracles' agreement on them are pinned here, where no GPU is needed."""
import numpy as np
import pytest

from oracle import pyref as P
from tests import extreme_operands as X

R = X.R
FULL = X.LIMB_FULL


def test_stored_word_classes_are_canonical_with_the_claimed_limbs():
    """every stored-word class is below r and has the limb pattern it claims, in the 29-bit limbs of x and of 32 x (f29_unpack / f29_unpack_shl5)"""
    for name, w in X.WORD_CLASSES.items():
        assert 0 <= w < R, name
        assert (32 * w) >> (X.LIMB_BITS * X.LIMBS) == 0, name         # 32 x fits the nine limbs
    assert R.bit_length() == 254 and X.TOP_LIMB_MAX == 0x30644E
    l = X.limbs29
    assert l(0) == [0] * 9 and l(1) == [1] + [0] * 8
    assert l((1 << 253) - 1) == [FULL] * 8 + [(1 << 21) - 1]
    assert l(32 * ((1 << 253) - 1)) == [FULL - 31] + [FULL] * 7 + [(1 << 26) - 1]
    assert l((1 << 232) - 1) == [FULL] * 8 + [0]
    assert l(32 * ((1 << 232) - 1)) == [FULL - 31] + [FULL] * 7 + [31]
    assert l(X.WORD_CLASSES["top"]) == [0] * 8 + [X.TOP_LIMB_MAX]
    assert l(32 * X.WORD_CLASSES["top"]) == [0] * 8 + [X.TOP_LIMB_MAX << 5]
    assert l(R - 1)[8] == X.TOP_LIMB_MAX and l(R - 2)[8] == X.TOP_LIMB_MAX
    assert l(R - 1)[0] == 1 << 28 and l(R - 2)[0] == (1 << 28) - 1   # r = 1 mod 2^28: r - 2 borrows through the low 28 bits
    assert R - 1 > X.WORD_CLASSES["top"] > (1 << 253) - 1 > (1 << 232) - 1
    # the value classes: -1, the two halves
    v = X.VALUE_CLASSES
    assert (v["v-1"] + 1) % R == 0 and 2 * v["v(r-1)/2"] % R == R - 1 and 2 * v["v(r+1)/2"] % R == 1
    # the word-space challenges stand for the words they name
    assert X.word_of(X.CHALLENGES["c:2^253-1"]) == (1 << 253) - 1 and X.word_of(X.CHALLENGES["c:r-1"]) == R - 1
    for k in (5, 10):      # ... and so do the ones named after their 2^(256 + k) image, the limb form the kernels keep in scalar registers
        assert X.word_of(X.CHALLENGES["c%d:2^253-1" % (256 + k)]) * (1 << k) % R == (1 << 253) - 1
        assert X.word_of(X.CHALLENGES["c%d:r-1" % (256 + k)]) * (1 << k) % R == R - 1
    assert len(set(X.CHALLENGES.values())) == len(X.CHALLENGES) == 12


def test_classes_round_trip_through_the_oracle(cref):
    """word -> value -> word and value -> word -> value through cref, and the helper's own Python conversion agrees with cref's"""
    names = list(X.ALL_WORDS)
    words = [X.ALL_WORDS[k] for k in names]
    arr = X.words_to_u64(words)
    assert X.u64_to_words(arr) == words
    vals = cref.fr_mont_to_ints(arr)
    assert vals == [X.value_of(w) for w in words] == [X.ALL_VALUES[k] for k in names]
    assert np.array_equal(cref.fr_ints_to_mont(vals), arr)
    assert all(0 <= x < R for x in vals)
    for k, val in X.VALUE_CLASSES.items():
        assert cref.fr_mont_to_ints(cref.fr_ints_to_mont([val])) == [val], k
        assert X.u64_to_words(cref.fr_ints_to_mont([val])) == [X.word_of(val)] == [X.ALL_WORDS[k]], k
    for k, c in X.CHALLENGES.items():
        assert 0 <= c < R and X.u64_to_words(cref.fr_ints_to_mont([c])) == [X.word_of(c)], k


def _columns(n, log_n):
    """name -> column of stored words: every pattern of the helper at length n"""
    w_inv = pow(P.fr_omega(log_n), -1, R)
    cols = {"const:" + k: X.constant(n, w) for k, w in X.ALL_WORDS.items()}
    cols.update({"alt:" + k: X.alternating(n, a, b) for k, (a, b) in X.ALT_PAIRS.items()})
    for k in X.MAXIMAL:
        for idx in sorted({0, n - 1, n // 2}):
            cols["onehot%d:%s" % (idx, k)] = X.one_hot(n, idx, X.ALL_WORDS[k])
        cols["geom:" + k] = X.geometric(n, X.ALL_WORDS[k], pow(w_inv, 3 % n, R))
    cols["sprinkled"] = X.sprinkled(n, 7 + log_n)
    return cols


def test_sprinkled_columns_hold_the_classes():
    for n in (1, 8, 64, 1000):
        col = X.sprinkled(n, n)
        assert len(col) == n and all(0 <= w < R for w in col)
        assert sum(w in set(X.ALL_WORDS.values()) for w in col) >= max(1, n // 8)
    assert X.sprinkled(64, 5) == X.sprinkled(64, 5) != X.sprinkled(64, 6)
    big = X.sprinkled(4096, 1)
    assert {w for w in big if w in set(X.ALL_WORDS.values())} == set(X.ALL_WORDS.values())   # every class is met
    assert max(big).bit_length() == 254                                                       # and the random rest reaches the top bit


@pytest.mark.parametrize("log_n", [3, 6])
def test_pyref_and_cref_agree_on_the_transform(cref, log_n):
    """oracle/pyref.py::ntt (Python integers) == oracle/cref.py::ntt_fr (the C restatement, Montgomery words) on every pattern"""
    n = 1 << log_n
    omega = P.fr_omega(log_n)
    w_m = cref.fr_ints_to_mont([omega])[0]
    for name, col in _columns(n, log_n).items():
        got = cref.fr_mont_to_ints(cref.ntt_fr(X.words_to_u64(col), w_m, log_n))
        assert got == P.ntt([X.value_of(w) for w in col], omega), name


@pytest.mark.parametrize("log_n", [3, 6])
def test_constant_columns_transform_to_exact_zeros(cref, log_n):
    """the constant column of every class gives n * a at index 0 and exactly n - 1 ZERO WORDS elsewhere from the oracle's transform: a lazy
    implementation meets k * p there, which its canonicalisation must turn into 0, never into p"""
    n = 1 << log_n
    w_m = cref.fr_ints_to_mont([P.fr_omega(log_n)])[0]
    for name, w in X.ALL_WORDS.items():
        out = cref.ntt_fr(X.words_to_u64(X.constant(n, w)), w_m, log_n)
        assert X.u64_to_words(out[:1]) == [n * w % R], name
        assert not out[1:].any() and out[1:].shape[0] == n - 1, name


def test_pyref_and_cref_agree_on_distribute_powers_and_scale(cref):
    """distribute_powers (a[i] *= g^i) and the scale (a[i] *= s) with g, s from the challenge classes, 0 and the word-space extremes included"""
    n = 64
    cols = _columns(n, 6)
    for cname, c in X.CHALLENGES.items():
        c_m = cref.fr_ints_to_mont([c])[0]
        for name in ("const:r-1", "const:2^253-1", "alt:w0|r-1", "sprinkled", "const:v(r+1)/2"):
            col = cols[name]
            vals = [X.value_of(w) for w in col]
            arr = X.words_to_u64(col)
            assert cref.fr_mont_to_ints(cref.fr_distribute_powers(arr, c_m)) == P.distribute_powers(vals, c), (cname, name)
            assert P.distribute_powers(vals, c) == P.coset_scale(vals, c), (cname, name)
            assert cref.fr_mont_to_ints(cref.fr_scale(arr, c_m)) == [v * c % R for v in vals], (cname, name)
            # linearity in word space, which the GPU tests' closed forms rest on
            assert X.u64_to_words(cref.fr_scale(arr, c_m)) == [w * c % R for w in col], (cname, name)
