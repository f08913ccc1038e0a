"""Operand classes and column patterns for the worst-case tests of the scalar-field (Fr) kernels (no GPU needed).

The Fr kernels run on the 9 x 29-bit lazy representation of paillier_halo2_amd/csrc/fp29.cuh, whose column accumulators have no carry-out:
their bound analyses speak of LIMBS (stored 256-bit Montgomery words cut into 29-bit pieces) and of VALUES (multiples of p a lazy value may
carry).  So there are two kinds of classes here:

  * stored-word classes: the 256-bit words as they lie in device memory, all canonical (below r) -- full limbs, an empty or a maximal top limb;
  * value classes: field VALUES (0, 1, 2, -1, +-1/2), converted to their Montgomery words.

Everything is a Python integer ("word": the stored Montgomery word, "value": the field element it stands for, word = value * 2^256 mod r)
or an (n, 4) uint64 array of words.  The transforms, the fold, the scalings and the division are LINEAR, so their closed forms hold in word
space with the constants (twiddles, challenges) in value space: word(a * c) = word(a) * c mod r.

tests/test_extreme_operands.py checks the classes themselves on the CPU; tests/test_gpu_extreme_operands.py drives the kernels with them."""
import numpy as np

from oracle import pyref as P

R = P.FR_R
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R)
LIMB_BITS, LIMBS = 29, 9
LIMB_FULL = (1 << LIMB_BITS) - 1
TOP_LIMB_MAX = R >> 232            # the ninth limb of r - 1 (22 bits)

# the 256-bit Montgomery words as they lie in device memory
WORD_CLASSES = {
    "w0": 0,                               # zero
    "w1": 1,                               # the smallest non-zero word
    "r-1": R - 1,                          # the largest legal word
    "2^253-1": (1 << 253) - 1,             # below r; eight full limbs, top limb 2^21 - 1; 32x is full as well
    "2^232-1": (1 << 232) - 1,             # low limbs full, top limb empty
    "top": TOP_LIMB_MAX << 232,            # only the top limb set, at its maximum
    "r-2": R - 2,                          # the neighbour of the largest legal word
}
# field values; their words come from word_of (== cref.fr_ints_to_mont, checked on the CPU)
VALUE_CLASSES = {
    "v0": 0,
    "v1": 1,
    "v2": 2,
    "v-1": R - 1,
    "v(r-1)/2": (R - 1) // 2,
    "v(r+1)/2": (R + 1) // 2,
}
MAXIMAL = ("r-1", "2^253-1")               # the constant maximal classes the quotient lines are filled with


def word_of(value: int) -> int:
    """field value -> its stored Montgomery word"""
    return value % R * MONT % R


def value_of(word: int) -> int:
    """stored Montgomery word -> the field value it stands for"""
    return word * MONT_INV % R


# every class as a stored word, and as the value that word stands for
ALL_WORDS = dict(WORD_CLASSES)
ALL_WORDS.update({k: word_of(v) for k, v in VALUE_CLASSES.items()})
ALL_VALUES = {k: value_of(w) for k, w in ALL_WORDS.items()}

# challenges (beta, gamma, theta, y, x, v, u, scale, coset generator): the value classes, and the values whose Montgomery WORD is extreme -- the
# host converts a challenge into limb form kept in scalar registers, so its worst case is in word space too ("c:").  That limb form is
# c * 2^(256 + k) mod r (pz_quotient.hip host_fr_shl: k = 5, the 261-domain image; k = 10 for beta in the grand products), and the cached
# power tables hold x^i * 2^261: the values whose IMAGE under that shift is an extreme word are classes as well ("c261:", "c266:")
CHALLENGES = dict(VALUE_CLASSES)
CHALLENGES.update({"c:2^253-1": value_of((1 << 253) - 1), "c:r-1": value_of(R - 1)})
for _k in (5, 10):
    for _nm, _w in (("2^253-1", (1 << 253) - 1), ("r-1", R - 1)):
        CHALLENGES["c%d:%s" % (256 + _k, _nm)] = value_of(_w) * pow(1 << _k, -1, R) % R

# alternating pairs of stored words the closed forms name
ALT_PAIRS = {"w0|r-1": (0, R - 1), "2^253-1|w0": ((1 << 253) - 1, 0), "r-1|2^253-1": (R - 1, (1 << 253) - 1)}


def limbs29(x: int, count: int = LIMBS):
    """the 29-bit limbs of x, least significant first (fp29.cuh's F29 layout)"""
    return [(x >> (LIMB_BITS * i)) & LIMB_FULL for i in range(count)]


# ------------------------------------------------------------------ integers <-> (n, 4) uint64
def words_to_u64(ws) -> np.ndarray:
    buf = b"".join(int(w).to_bytes(32, "little") for w in ws)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).copy()


def u64_to_words(arr):
    b = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def word_u64(w: int) -> np.ndarray:
    return words_to_u64([w])[0]


# ------------------------------------------------------------------ column patterns (lists of stored words)
def constant(n: int, w: int):
    return [w] * n


def alternating(n: int, a: int, b: int):
    """a at the even indices, b at the odd ones"""
    return [a if i % 2 == 0 else b for i in range(n)]


def one_hot(n: int, idx: int, w: int, fill: int = 0):
    """w at index idx (0, n - 1, or a block boundary the caller passes), fill elsewhere"""
    assert 0 <= idx < n
    col = [fill] * n
    col[idx] = w
    return col


def geometric(n: int, c: int, ratio: int):
    """c * ratio^i: ratio a field VALUE (for the transforms omega^-j, so that a single output is non-zero), c a stored word"""
    out, cur = [], c % R
    for _ in range(n):
        out.append(cur)
        cur = cur * ratio % R
    return out


def sprinkled_u64(n: int, seed: int) -> np.ndarray:
    """(n, 4) uint64: uniformly random canonical words with every eighth element (in seeded positions; at least one) drawn from the classes"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)                    # below 2^254
    # a word at or above r (one in four of those above 2^253) loses its two top bits: the rest is uniform below r up to that fold
    top, rtop = a[:, 3], np.uint64(R >> 192)
    over = top >= rtop                                          # conservative: the top 64-bit word decides
    a[over, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
    k = max(1, n // 8)
    pos = rng.choice(n, size=k, replace=False)
    cls = words_to_u64(list(ALL_WORDS.values()))
    a[pos] = cls[rng.integers(0, len(cls), size=k)]
    return a


def sprinkled(n: int, seed: int):
    return u64_to_words(sprinkled_u64(n, seed))
