"""Structured steps for the witness expansion (K4, csrc/pz_witness.hip) and a restatement of its carry and borrow chains in Python
integers.  The catalogue: shapes (limbs, limb width, lookup width) at the edges of the scan's terms per lane,
of the limb cutter and of the range-check tails; moduli of L W bits or fewer; honest steps (q, r = divmod(a b, n)) over structured
operands; inconsistent steps, which the device must expand to the same unsatisfied witness as the reference would.  The restatement
walks a step the way is_equal_muled and the r < n comparison do and says what a step visits (the census).  Pure Python; the product
must not import this module."""
import random
from typing import Dict, List, NamedTuple, Tuple

# (L, W, lb).  L at the edges of PER = ceil((2 L - 1) / 64): 32 | 33, 64 | 65, 96 | 97, 128; W: 16 and 90 (the bounds), 17, 32 and 63 (limbs
# that straddle a word, begin at bit 0 or end at bit 63), 64, 65 and 88 (the `wide` arm); lb: 4 and 32 (the bounds) and the values that give
# W % lb and cb % lb each of 0, 1, more -- in every class of shapes (PER = 1 | 2 | 3 | 4, one line each below).  L = 128 only at W = 64.
SHAPES = (
    (2, 16, 4), (2, 64, 22), (2, 88, 32), (2, 90, 11), (3, 32, 8), (4, 64, 15), (4, 64, 21), (4, 64, 22), (6, 88, 15), (8, 90, 32),
    (32, 63, 9),
    (33, 64, 14), (33, 65, 8), (64, 65, 13),
    (65, 17, 8), (65, 64, 16), (96, 64, 18),
    (97, 64, 13), (97, 64, 9), (97, 17, 4), (128, 64, 16),
)
# just outside what make_params admits; admitted() gives the status.  (128, 90, .) is NOT outside: 2 W + ceil(log2 L) + 3 is 190 there,
# the largest value any L <= 128, W <= 90 reaches, so that rule never binds -- the widest shape stands among the edges as one make_params takes
EDGES = ((1, 64, 15), (129, 64, 15), (4, 15, 5), (4, 91, 15), (128, 90, 15), (4, 64, 3), (4, 64, 33), (4, 16, 16), (4, 32, 32), (2, 20, 32))
WIDEST = (128, 90, 15)
MODULI = ("all_ones", "pow2_plus1", "top2", "alt", "zero_mid", "random")


def ceil_log2(x: int) -> int:
    return (x - 1).bit_length()


def admitted(L: int, W: int, lb: int) -> str:
    """make_params' documented rules: '' if the shape is taken, else the status"""
    if W < 16 or W > 90 or L < 2 or L > 128:
        return "unsupported"
    if lb < 4 or lb > 32:
        return "invalid"
    if 2 * W + ceil_log2(L) + 3 > 192:
        return "unsupported"
    if -(-W // lb) < 2:
        return "invalid"
    return ""


def per(L: int) -> int:
    """terms of a convolution row one lane of the scan owns"""
    return (2 * L - 1 + 63) // 64


def max_term(L: int, W: int) -> int:
    m = (1 << W) - 1
    return L * m * m + m


def carry_bits(L: int, W: int) -> int:
    return (2 * max_term(L, W)).bit_length() - W


def tail(bits: int, lb: int) -> int:
    """the range check's tail pattern: 0 (no tail gate), 1 (the last digit is one bit), 2 (shifted last digit, one more lookup)"""
    return min(bits % lb, 2)


def step_cap(L: int):
    """steps per modulus: all of them for small shapes, fewer where one step of the reference model costs 0.05 to 0.2 s.  The first 12
    hold every census class, the first 16 every inconsistent step, the ones after them are honest"""
    return None if L <= 8 else 24 if L <= 65 else 16 if L <= 96 else 12


def limbs(x: int, L: int, W: int) -> List[int]:
    assert x >> (L * W) == 0
    return [(x >> (W * i)) & ((1 << W) - 1) for i in range(L)]


def ones(L: int, W: int) -> int:
    return (1 << (L * W)) - 1


def alt(L: int, W: int) -> int:
    """limbs alternating all ones / zero, from limb 0"""
    return sum(((1 << W) - 1) << (W * i) for i in range(0, L, 2))


def one_hot(L: int, W: int, pos: int) -> int:
    """one limb all ones, the others zero"""
    return ((1 << W) - 1) << (W * pos)


def modulus(name: str, L: int, W: int) -> int:
    """an odd modulus of at most L W bits"""
    bits = L * W
    rng = random.Random(0x7734 + 1000 * L + W)
    if name == "all_ones":
        return (1 << bits) - 1
    if name == "pow2_plus1":
        return (1 << (bits - 1)) + 1
    if name == "top2":
        return (2 << (W * (L - 1))) + 1
    if name == "alt":
        return alt(L, W)
    if name == "zero_mid":
        v = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        return v & ~one_hot(L, W, L // 2)
    assert name == "random"
    rng.getrandbits(bits)
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def operands(n: int, L: int, W: int) -> Dict[str, int]:
    """the operand classes by name; every value has at most L limbs, the ones marked `raw` need not be below n"""
    full = ones(L, W)
    out = {"0": 0, "1": 1, "n-1": n - 1, "n-2": n - 2, "n/2": n // 2, "ones": full % n, "ones_raw": full, "alt": alt(L, W) % n,
           "alt_raw": alt(L, W), "hot0": one_hot(L, W, 0) % n, "hot_mid": one_hot(L, W, L // 2) % n, "hot_top": one_hot(L, W, L - 1) % n,
           "hot_top_raw": one_hot(L, W, L - 1)}
    return out


class Step(NamedTuple):
    name: str
    a: int
    b: int
    q: int
    r: int
    honest: bool


def _honest(name: str, a: int, b: int, n: int) -> Step:
    q, r = divmod(a * b, n)
    return Step(name, a, b, q, r, True)


def final_only(L: int, W: int) -> Tuple[int, int]:
    """(a, b) with a b = 2^(W (2 L - 1)): against q = r = 0 every limb's low W bits agree and only the last carry differs"""
    k = W // 2
    return 1 << (W * (L - 1) + k), 1 << (W * (L - 1) + W - k)


def steps(name: str, L: int, W: int, cap=None) -> List[Step]:
    """the steps under modulus `name`, the ones every shape runs first; `cap` cuts the list (at 12 it still holds one step of every
    census class)"""
    n = modulus(name, L, W)
    full = ones(L, W)
    ops = operands(n, L, W)
    fits = lambda a, b: a * b // n <= full

    def pair(x: str, y: str) -> Step:
        a, b = ops.get(x + "_raw", ops[x]), ops.get(y + "_raw", ops[y])
        if not fits(a, b):
            a, b = ops[x], ops[y]
        return _honest("%s*%s" % (x, y), a, b, n)

    base = pair("n-1", "n-1")
    low = pair("n-1", "1")
    fa, fb = final_only(L, W)
    out = [
        pair("ones", "ones"), base, low, pair("alt", "alt"),
        Step("r+1", base.a, base.b, base.q, base.r + 1, False),
        Step("r+hot_mid", base.a, base.b, base.q, base.r + (1 << (W * (L // 2))), False),
        Step("q+1", base.a, base.b, min(base.q + 1, full), base.r, False),
        Step("r=n", low.a, low.b, low.q, n, False),
        Step("r=ones", low.a, low.b, low.q, full, False),
        Step("0*0|q=r=ones", 0, 0, full, full, False),
        Step("ones*ones|q=r=0", full, full, 0, 0, False),
        Step("final_only", fa, fb, 0, 0, False),
    ]
    mid = pair("n/2", "n-2")
    more = [
        Step("r-1", mid.a, mid.b, mid.q, mid.r - 1 if mid.r else 1, False),
        Step("q-1", mid.a, mid.b, mid.q - 1 if mid.q else 2, mid.r, False),
        Step("q<->r", mid.a, mid.b, mid.r, mid.q, False),
    ]
    hot = 1 << (W * (L // 2))
    if base.r + n >= hot:      # a b - (q - 1) n - (r + n - hot) = +hot: the difference of the other sign at a middle limb
        more.append(Step("r-hot_mid", base.a, base.b, base.q - 1, base.r + n - hot, False))
    names = [k for k in ops if not k.endswith("_raw")]
    more += [pair(x, x) for x in names] + [pair(x, names[(i + 1) % len(names)]) for i, x in enumerate(names)] + [pair("1", x) for x in names]
    seen = {s[1:5] for s in out}
    for s in more:
        if s[1:5] not in seen:
            seen.add(s[1:5])
            out.append(s)
    for s in out:
        assert 0 <= min(s.a, s.b, s.q, s.r) and max(s.a, s.b, s.q, s.r) <= full, s.name
        assert not s.honest or (s.a * s.b == s.q * n + s.r and s.r < n), s.name
    return out[:cap] if cap else out


# ---------------------------------------------------------------------------------------------------------------- the restated chains
class Walk(NamedTuple):
    pab: List[int]          # product limbs of a b (2 L - 1)
    qnr: List[int]          # product limbs of q n, r added
    carries: List[int]      # the carry out of every limb
    e: List[int]            # per limb: the low W bits agree; then the final carry comparison
    diffs: List[int]        # per is_equal of the chain: x - y
    eq: int                 # the running bit at the end
    borrow_in: List[int]    # r < n: the borrow into every limb
    nb: List[int]           # n_i + borrow
    borrow: int             # the final borrow (1 = r < n)


def walk(a: int, b: int, q: int, r: int, n: int, L: int, W: int) -> Walk:
    """is_equal_muled(a b, q n + r) and r < n as the kernel's serial lane walks them"""
    B = 1 << W
    D = 2 * L - 1
    al, bl, ql, rl, nl = (limbs(v, L, W) for v in (a, b, q, r, n))
    conv = lambda x, y: [sum(x[j] * y[i - j] for j in range(max(0, i - L + 1), min(i, L - 1) + 1)) for i in range(D)]
    pab, qnr = conv(al, bl), conv(ql, nl)
    for i in range(L):
        qnr[i] += rl[i]
    MAX = max_term(L, W)
    carry = acc = 0
    carries, e, diffs = [], [], []
    for i in range(D):
        s = pab[i] - qnr[i] + carry + MAX
        assert s >= 0, "|ab_i - (qn + r)_i| <= MAX and the carry is not negative"
        t = acc + MAX
        e.append(1 if s % B == t % B else 0)
        diffs.append(s % B - t % B)
        carry, acc = s >> W, t >> W
        carries.append(carry)
    e.append(1 if carry == acc else 0)
    diffs.append(carry - acc)
    borrow, borrow_in, nbs = 0, [], []
    for i in range(L):
        borrow_in.append(borrow)
        nbs.append(nl[i] + borrow)
        borrow = 1 if rl[i] < nl[i] + borrow else 0
    return Walk(pab, qnr, carries, e, diffs, int(all(e)), borrow_in, nbs, borrow)


CENSUS = ("limb>=2^128", "nb=2^W", "r_i=n_i|b=0", "r_i=n_i|b=1", "final_borrow=0", "e0@0", "e0@mid", "e0@final", "diff<0", "diff>0",
          "carry_top_digit", "limb_tail0", "limb_tail1", "limb_tail2", "carry_tail0", "carry_tail1", "carry_tail2")


def census_of(s: Step, n: int, L: int, W: int, lb: int) -> Dict[str, int]:
    """what one step visits: 1 or 0 per census class, and per slot of the scan's last lane"""
    w = walk(s.a, s.b, s.q, s.r, n, L, W)
    rl, nl = limbs(s.r, L, W), limbs(n, L, W)
    D, P = 2 * L - 1, per(L)
    first = w.e.index(0) if 0 in w.e else -1
    cb = carry_bits(L, W)
    top = lb * (-(-cb // lb) - 1)
    out = {
        "limb>=2^128": int(any(v >> 128 for v in w.pab + w.qnr)),
        "nb=2^W": int(any(v == 1 << W for v in w.nb)),
        "r_i=n_i|b=0": int(any(rl[i] == nl[i] and w.borrow_in[i] == 0 for i in range(L))),
        "r_i=n_i|b=1": int(any(rl[i] == nl[i] and w.borrow_in[i] == 1 for i in range(L))),
        "final_borrow=0": int(w.borrow == 0),
        "e0@0": int(first == 0),
        "e0@mid": int(0 < first < D),
        "e0@final": int(first == D),
        "diff<0": int(any(d < 0 for d in w.diffs)),
        "diff>0": int(any(d > 0 for d in w.diffs)),
        "carry_top_digit": int(any(c >> top for c in w.carries[:-1])),
    }
    for t in range(3):          # the tail pattern is the shape's: every step of the shape runs it, L times per limb check, D - 1 per carry
        out["limb_tail%d" % t] = int(tail(W, lb) == t)
        out["carry_tail%d" % t] = int(tail(cb, lb) == t)
    al, bl = limbs(s.a, L, W), limbs(s.b, L, W)
    for t in range(P):
        hit = 0
        for i in range(D):
            j = i // P * P + t
            if j <= i and j < L and i - j < L and al[j] and bl[i - j]:
                hit = 1
                break
        out["slot%d" % t] = hit
    return out


def census(shapes=SHAPES) -> Dict[int, Dict[str, int]]:
    """per class of shapes (PER = 1 .. 4): the steps of the catalogue, cut as the GPU tests cut them, that visit each census class"""
    table: Dict[int, Dict[str, int]] = {}
    for L, W, lb in shapes:
        row = table.setdefault(per(L), {})
        for name in MODULI:
            n = modulus(name, L, W)
            for s in steps(name, L, W, step_cap(L)):
                for k, v in census_of(s, n, L, W, lb).items():
                    row[k] = row.get(k, 0) + v
                row["steps"] = row.get("steps", 0) + 1
    return table


def tails(shapes=SHAPES) -> Dict[int, Dict[str, List[int]]]:
    """per class of shapes: the shapes per tail pattern [none, one bit, more] of the two range checks (functions of the shape alone)"""
    table: Dict[int, Dict[str, List[int]]] = {}
    for L, W, lb in shapes:
        out = table.setdefault(per(L), {"limb": [0, 0, 0], "carry": [0, 0, 0]})
        out["limb"][tail(W, lb)] += 1
        out["carry"][tail(carry_bits(L, W), lb)] += 1
    return table


# ---------------------------------------------------------------------------------------------------------------- whole circuits
MERSENNE_150 = ((1 << 61) - 1) * ((1 << 89) - 1)       # tests/k3_operands.py MERSENNE[0]: 150 bits


def circuit_keys(bits: int) -> Dict[str, int]:
    """odd keys of at most `bits` bits; the Mersenne product where it fits"""
    out = {"all_ones": (1 << bits) - 1, "pow2_plus1": (1 << (bits - 1)) + 1,
           "alt": sum(0xFFFF << (32 * i) for i in range(-(-bits // 32))) & ((1 << bits) - 1)}
    if bits >= 150:
        out["mersenne"] = MERSENNE_150
    return out


def break_points(mask, max_rows: int):
    """halo2-lib's column break rule with the assertion it makes on the way: a gate that would straddle the break moves to the next
    column with its first cell; the walk refuses (None) a stream in which a gate began one or two cells before such a cell inside
    the column, since gates overlap by exactly three cells or not at all"""
    n = len(mask)
    starts, s = [0], 0
    while True:
        end = None
        for i in range(s, n):
            r = i - s
            if (mask[i] and r + 4 > max_rows) or r >= max_rows - 1:
                end = i
                break
        if end is None:
            break
        if mask[end] and end - s < max_rows - 1:
            for back in (1, 2):
                if end - back > s and mask[end - back]:
                    return None
        s = end
        starts.append(s)
    starts.append(n)
    return starts
