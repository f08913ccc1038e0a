"""Test helper (not product code): the halo2 wire format of DESIGN.md section 15.2 in Python integers.  Shares nothing with
paillier_halo2_amd: its own moduli, its own square root (pow), its own statement of the proof and key layouts.

G1 point, 32 bytes: canonical x little-endian, bit 7 of byte 31 = y & 1, bit 6 of byte 31 zero, the identity 32 zero bytes.
Scalar, 32 bytes: the canonical value below r.
Proof: commitments (without W1, W2) | evaluations (without h(x)) | W1 | W2.
Key file: "PZVK", u32 version 1, k, blinding_factors, n_adv, n_lk, then fixed and sigma commitments compressed."""
import struct

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT = 1 << 256
assert P % 4 == 3 and pow(3, (P - 1) // 2, P) != 1          # the (p+1)/4 root; 3 is not a square, so x = 0 is never on the curve
assert bin((P + 1) // 4).count("1") == 109 and ((P + 1) // 4).bit_length() == 252

OK, NOT_CANONICAL, OFF_CURVE = 0, 1, 2

# the order the transcript absorbs a proof in (family, points per element)
COMMITMENTS = ("advice", "lookup_advice", "perm_inputs", "perm_tables", "perm_z", "lookup_z", "random", "h")
EVALS = ("advice", "lookup_advice", "constants", "fixed", "sigma", "perm_z", "lookup_z", "perm_inputs", "perm_tables", "random")
TAIL = ("w1", "w2")


def compress(pt) -> bytes:
    """pt: (x, y) canonical integers, or None for the identity"""
    if pt is None:
        return bytes(32)
    x, y = pt
    assert 0 <= x < P and 0 <= y < P and (y * y - x * x * x - 3) % P == 0
    return (x | (y & 1) << 255).to_bytes(32, "little")


def decompress(b: bytes):
    """-> (status, point): point is (x, y), None for the identity and for a refused encoding"""
    assert len(b) == 32
    v = int.from_bytes(b, "little")
    sign = v >> 255
    x = v & ((1 << 255) - 1)
    if x >= P or x >> 254:
        return NOT_CANONICAL, None
    if x == 0 and sign == 0:
        return OK, None
    rhs = (x * x * x + 3) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return OFF_CURVE, None
    if y & 1 != sign:
        y = P - y
    return OK, (x, y)


def scalar_bytes(v: int) -> bytes:
    assert 0 <= v < R
    return v.to_bytes(32, "little")


def scalar_from_bytes(b: bytes):
    v = int.from_bytes(b, "little")
    return (NOT_CANONICAL, None) if v >= R else (OK, v)


# ---- the ABI's Montgomery words <-> integers -----------------------------------------------------------------------------------------
def _word_ints(words, per):
    flat = [int(w) for w in getattr(words, "reshape", lambda *_: words)(-1)]
    assert len(flat) % per == 0
    vals = [sum(flat[i + j] << (64 * j) for j in range(4)) for i in range(0, len(flat), 4)]
    return vals


def points_from_words(words):
    """(count, 8) Montgomery words -> [(x, y) or None]"""
    inv = pow(MONT, -1, P)
    v = [c * inv % P for c in _word_ints(words, 8)]
    return [None if (v[i] == 0 and v[i + 1] == 0) else (v[i], v[i + 1]) for i in range(0, len(v), 2)]


def scalars_from_words(words):
    inv = pow(MONT, -1, R)
    return [c * inv % R for c in _word_ints(words, 4)]


def point_words(pt):
    """(x, y) or None -> 8 Montgomery words as integers"""
    x, y = (0, 0) if pt is None else (pt[0] * MONT % P, pt[1] * MONT % P)
    return [(c >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for c in (x, y) for j in range(4)]


# ---- proofs and keys ------------------------------------------------------------------------------------------------------------------
def proof_counts(n_adv: int, n_lk: int):
    """-> (n_own, n_ev): a proof's commitments (W1, W2 included) and pz_proof_evaluate's elements (h(x) included)"""
    m = n_adv + n_lk + 1
    n_sets = -(-m // 2)
    n_own = n_adv + 4 * n_lk + n_sets + 6
    n_ev = 4 * n_adv + n_lk + 1 + (n_adv + 2) + m + 3 * n_sets + 2 * n_lk + 2 * n_lk + n_lk + 1 + 1
    return n_own, n_ev


def proof_size(n_adv: int, n_lk: int) -> int:
    n_own, n_ev = proof_counts(n_adv, n_lk)
    return 32 * (n_own + n_ev - 1)


def proof_bytes(commitments, evals) -> bytes:
    """commitments / evals: prover.Proof-shaped dicts of Montgomery word arrays"""
    out = b"".join(compress(pt) for f in COMMITMENTS for pt in points_from_words(commitments[f]))
    out += b"".join(scalar_bytes(v) for f in EVALS for v in scalars_from_words(evals[f]))
    out += b"".join(compress(pt) for f in TAIL for pt in points_from_words(commitments[f]))
    return out


def vk_bytes(k: int, blinding_factors: int, n_adv: int, n_lk: int, fixed, sigma) -> bytes:
    pts = points_from_words(fixed) + points_from_words(sigma)
    assert len(pts) == (n_adv + 2) + (n_adv + n_lk + 1)
    return b"PZVK" + struct.pack("<5I", 1, k, blinding_factors, n_adv, n_lk) + b"".join(compress(p) for p in pts)


# ---- a little curve arithmetic for test inputs ------------------------------------------------------------------------------------------
def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2 and (y1 + y2) % P == 0:
        return None
    lam = (3 * x1 * x1 * pow(2 * y1, -1, P) if a == b else (y2 - y1) * pow(x2 - x1, -1, P)) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def mul(k: int, pt=(1, 2)):
    acc = None
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc
