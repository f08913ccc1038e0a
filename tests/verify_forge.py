"""TEST INFRASTRUCTURE: proofs CONSTRUCTED TO VERIFY for any verifying-key shape, without a prover.

The tests know the SRS scalar s, and every commitment is [c] G with a known log c.  Then for any shape (A, Lk, n_instance, k, bf):
random evaluations and random logs, the stated h(x) set to what the oracle's verifier expects, and the one log that enters no
challenge -- W2 is not absorbed before sh_u -- solved so that the opening identity a + s b == 0 (mod r) holds, where

    a = sum_k v^k z_k ( sum_j y^j c_kj - R_k(u) ) - Z_T(u) w1 + z_0 u w2        (the log of SHPLONK's A; g0 = G, so [R_k(u)] has log R_k(u))
    b = - z_0 w2                                                              (the log of B)

A verifier accepts such a proof exactly when every value it derives (challenges, Lagrange values, h(x), every scalar of the final
multi-scalar multiplication) is the value computed here, and its A and B are [a] G and [b] G.

Everything is Python integers on top of the oracle (oracle/pyref.py, oracle/verifier.py) and tests/public_ref.py.  Of the product only
prover.query_layout (the order of the queries, which the oracle's shplonk_check takes from there too) is used: the product's verifier
(verifier._terms, verifier.constraint_expression, csrc/) is what this file is held against, never what it calls.  No GPU code: the
caller supplies `points`, the map from logs to affine words ([c] G; c = 0 is the identity (0, 0))."""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import pyref as P
from oracle import verifier as V
from tests import public_ref as PR

R = P.FR_R
Q = P.FQ_P
CHUNK = 2                                 # permutation columns per grand product
DELTA = pow(P.FR_GENERATOR, 1 << P.FR_S, R)    # halo2curves' Fr::DELTA
H_PIECES = 3
# include/pz.h, pz_verify_batch: the order of a proof's words
COMMITMENT_ORDER = ("advice", "lookup_advice", "perm_inputs", "perm_tables", "perm_z", "lookup_z", "random", "h", "w1", "w2")
EVAL_ORDER = ("advice", "lookup_advice", "constants", "fixed", "sigma", "perm_z", "lookup_z", "perm_inputs", "perm_tables", "random", "h")
SPECIAL_VALUES = (0, 1, R - 1)


@dataclass(frozen=True)
class Shape:
    A: int
    Lk: int
    n_instance: int
    k: int
    bf: int
    n_public: int = 0

    @property
    def m(self) -> int:
        return self.A + self.Lk + 1 + self.n_instance

    @property
    def S(self) -> int:
        return -(-self.m // CHUNK)

    @property
    def NL(self) -> int:
        """lines of the constraint expression"""
        return self.A + 1 + 2 * self.S + 5 * self.Lk

    @property
    def M0(self) -> int:
        """members of the first query set (the one opened at x alone)"""
        return self.A + 2 * self.Lk + self.m + 4

    @property
    def n_own(self) -> int:
        return self.A + 4 * self.Lk + self.S + 6

    def commitment_counts(self) -> Dict[str, int]:
        A, Lk, S = self.A, self.Lk, self.S
        return dict(zip(COMMITMENT_ORDER, (A, Lk, Lk, Lk, S, Lk, 1, H_PIECES, 1, 1)))

    def eval_shapes(self) -> Dict[str, Tuple[int, int]]:
        A, Lk, S, m = self.A, self.Lk, self.S, self.m
        return dict(zip(EVAL_ORDER, ((A, 4), (Lk, 1), (1, 1), (A + 2, 1), (m, 1), (S, 3), (Lk, 2), (Lk, 2), (Lk, 1), (1, 1), (1, 1))))

    def rotation_points(self, x: int) -> List[int]:
        """x, wx, w^2 x, w^3 x, w^-(bf+1) x, w^-1 x"""
        w = P.fr_omega(self.k)
        return [x % R, x * w % R, x * pow(w, 2, R) % R, x * pow(w, 3, R) % R, x * pow(w, -(self.bf + 1), R) % R, x * pow(w, -1, R) % R]

    def degenerate(self) -> bool:
        """bf = 2^k - 2: w^-(bf+1) = w, so the set {x, wx, w^-(bf+1) x} of the chained permutation products names one point twice and no
        interpolation R_k exists.  (halo2 itself refuses such a domain: it wants blinding_factors + 3 <= 2^k rows.)"""
        return self.bf + 2 == 1 << self.k


def mont_words(v: int, mod: int = R) -> List[int]:
    v = (v % mod) * (1 << 256) % mod
    return [(v >> (64 * j)) & P.MASK64 for j in range(4)]


def int_words(v: int) -> List[int]:
    """a 256-bit integer as it stands: 4 little-endian words (no reduction, no Montgomery factor)"""
    return [(v >> (64 * j)) & P.MASK64 for j in range(4)]


def words_int(w) -> int:
    return sum(int(x) << (64 * j) for j, x in enumerate(w))


def eval_words(rows: Sequence[Sequence[int]]) -> np.ndarray:
    return np.array([[mont_words(v) for v in row] for row in rows], dtype=np.uint64).reshape(len(rows), -1, 4)


@dataclass
class Key:
    shape: Shape
    fixed_log: List[int]
    sigma_log: List[int]
    fixed: np.ndarray          # (A + 2, 8)
    sigma: np.ndarray          # (m, 8)


@dataclass
class Forged:
    key: Key
    seed: bytes
    instances: Optional[List[int]]
    clog: Dict[str, List[int]]             # the commitments' logs, w2 included
    com: Dict[str, np.ndarray]             # their words (count, 8), as sent
    evi: Dict[str, List[List[int]]]        # the evaluations as integers, the stated h(x) included
    ev: Dict[str, np.ndarray]              # (count, points, 4) Montgomery words, as sent
    ch: Dict[str, int]                     # the challenges of the words as sent
    h: int                                 # the oracle's expected h(x)
    solved: bool
    w2: int
    a: Optional[int]                       # log of A (None for a degenerate shape: no opening exists)
    b: Optional[int]
    a_wo_w2: Optional[int] = None
    z0: Optional[int] = None
    extra: dict = field(default_factory=dict)

    @property
    def shape(self) -> Shape:
        return self.key.shape

    def words(self) -> np.ndarray:
        """the proof in pz_verify_batch's layout"""
        return np.concatenate([np.asarray(self.com[f], dtype=np.uint64).reshape(-1) for f in COMMITMENT_ORDER] +
                              [np.asarray(self.ev[f], dtype=np.uint64).reshape(-1) for f in EVAL_ORDER])

    def h_words(self) -> np.ndarray:
        return np.array(mont_words(self.h), dtype=np.uint64)

    def holds(self, s_tox: int) -> bool:
        return (self.a + s_tox * self.b) % R == 0

    def twin(self, rng, points: Callable, defect: Optional[int] = None, s_tox: Optional[int] = None) -> "Forged":
        """the same proof with another W2: the same transcript, challenges and h(x), another A and B, and an opening that does not hold.
        W2 is random, or (defect, with the SRS scalar) the one for which a + s b == defect (mod r), defect != 0"""
        t = copy.copy(self)
        t.clog = dict(self.clog)
        t.com = dict(self.com)
        if defect is None:
            t.w2 = rng.randrange(1, R)
            while t.w2 == self.w2:
                t.w2 = rng.randrange(1, R)
        else:
            assert defect % R != 0
            t.w2 = (defect - self.a_wo_w2) * pow(self.z0 * (self.ch["sh_u"] - s_tox) % R, -1, R) % R
        t.clog["w2"] = [t.w2]
        t.com["w2"] = np.asarray(points([t.w2]), dtype=np.uint64).reshape(1, 8)
        t.solved = False
        if self.a_wo_w2 is not None:
            t.a, t.b = _ab(self.a_wo_w2, self.z0, self.ch["sh_u"], t.w2)
        return t


def _ab(a_wo_w2: int, z0: int, u: int, w2: int) -> Tuple[int, int]:
    return (a_wo_w2 + z0 * u % R * w2) % R, (-z0 * w2) % R


def forge_key(shape: Shape, rng, points: Callable) -> Key:
    fl = [rng.randrange(1, R) for _ in range(shape.A + 2)]
    sl = [rng.randrange(1, R) for _ in range(shape.m)]
    w = np.asarray(points(fl + sl), dtype=np.uint64).reshape(-1, 8)
    return Key(shape, fl, sl, w[:shape.A + 2].copy(), w[shape.A + 2:].copy())


def forge(shape: Shape, rng, seed: bytes, s_tox: int, points: Callable, *, key: Optional[Key] = None, solve: bool = True,
          specials: Optional[int] = None, identities: Sequence[Tuple[str, int]] = (), tamper: Optional[Callable] = None) -> Forged:
    """-> a proof of `shape` under `key` (a fresh forge_key if None) that verifies (solve = False: a random W2, a rejecting opening).
    specials: an integer turn t -- slot j (j < 3, in flat order) of evaluation family number f holds SPECIAL_VALUES[(j + t + f) % 3], so
    three proofs with turns 0, 1, 2 put 0, 1 and r - 1 into every family, the one-slot families included, and neighbouring families
    (a lookup's permuted input and table, say) do not hold the same value in the same slot, which would zero their lines.
    identities: (family, index) commitments with log 0.  tamper(com, ev): edits the words in place after they are formed and before
    the transcript is replayed, so the challenges (and the solved W2) are those of the words as sent."""
    sh = shape
    if key is None:
        key = forge_key(sh, rng, points)
    A, Lk, m, S, k = sh.A, sh.Lk, sh.m, sh.S, sh.k
    clog = {f: [rng.randrange(1, R) for _ in range(n)] for f, n in sh.commitment_counts().items() if f != "w2"}
    for f, i in identities:
        clog[f][i] = 0
    evi = {f: [[rng.randrange(R) for _ in range(q)] for _ in range(n)] for f, (n, q) in sh.eval_shapes().items() if f != "h"}
    if specials is not None:
        for fi, f in enumerate(EVAL_ORDER[:-1]):
            rows = evi[f]
            q = len(rows[0])
            for j in range(min(3, len(rows) * q)):
                rows[j // q][j % q] = SPECIAL_VALUES[(j + specials + fi) % 3]
    instances = [rng.randrange(R) for _ in range(sh.n_public)] if sh.n_instance else None
    fams = [f for f in COMMITMENT_ORDER if f != "w2"]
    flat = np.asarray(points([c for f in fams for c in clog[f]]), dtype=np.uint64).reshape(-1, 8)
    com, o = {}, 0
    for f in fams:
        com[f] = flat[o:o + len(clog[f])].copy()
        o += len(clog[f])
    ev = {f: eval_words(rows) for f, rows in evi.items()}
    if tamper is not None:
        tamper(com, ev)
    if sh.n_instance:
        ch = PR.replay_challenges_pub(seed, instances, com, ev)
        inst_x = PR.instance_eval(k, instances, ch["x"])
    else:
        ch = V.replay_challenges(seed, com, ev)
        inst_x = None
    x, sy, sv, su = ch["x"], ch["sh_y"], ch["sh_v"], ch["sh_u"]
    h = PR.expected_h_pub(k, sh.bf, A, Lk, CHUNK, evi, ch["beta"], ch["gamma"], ch["y"], x, DELTA, inst_x)
    evi["h"] = [[h]]
    ev["h"] = eval_words(evi["h"])
    out = Forged(key, bytes(seed), instances, clog, com, evi, ev, ch, h, solve, 0, None, None)
    if sh.degenerate():
        if solve:
            raise ValueError("blinding_factors = 2^k - 2: a query set names one point twice, no opening can be constructed")
        w2 = rng.randrange(1, R)
    else:
        from paillier_halo2_amd import prover

        pts = sh.rotation_points(x)
        xn = pow(x, 1 << k, R)
        log_of = {"fixed": key.fixed_log, "sigma": key.sigma_log, "h": [sum(pow(xn, p, R) * c for p, c in enumerate(clog["h"])) % R]}
        zt = 1
        for t in pts:
            zt = zt * (su - t) % R
        a, z0 = 0, None
        for kk, (idx, members) in enumerate(prover.query_layout(A, Lk, m, S)):
            zk = 1
            for t, pt in enumerate(pts):
                if t not in idx:
                    zk = zk * (su - pt) % R
            if kk == 0:
                z0 = zk
            xs = [pts[i] for i in idx]
            folded, csum, yj = [0] * len(xs), 0, 1
            for f, i in members:
                for q in range(len(xs)):
                    folded[q] = (folded[q] + yj * evi[f][i][q]) % R
                csum = (csum + yj * log_of.get(f, clog.get(f))[i]) % R
                yj = yj * sy % R
            rk_u = P.poly_eval(P.interpolate(xs, folded), su)
            a = (a + pow(sv, kk, R) * zk % R * (csum - rk_u)) % R
        a = (a - zt * clog["w1"][0]) % R
        den = z0 * (su - s_tox) % R                          # a_wo_w2 + z0 u w2 - s z0 w2 == 0
        if solve and den == 0:
            raise ValueError("u == s: choose another seed")
        w2 = (-a) * pow(den, -1, R) % R if solve else rng.randrange(1, R)
        out.a_wo_w2, out.z0 = a, z0
        out.a, out.b = _ab(a, z0, su, w2)
    out.w2 = w2
    clog["w2"] = [w2]
    com["w2"] = np.asarray(points([w2]), dtype=np.uint64).reshape(1, 8)
    return out


# The key shapes of the verifier's tests.  With m = A + Lk + 1 + n_instance, S = ceil(m / 2): the expression has NL = A + 1 + 2 S + 5 Lk
# lines and the first query set M0 = A + 2 Lk + m + 4 members; the device gives each of 256 lanes a contiguous share of either, so the
# sizes around 256 are where a lane's share goes from one item to two (and below 256, where most lanes have none).
# NL = 257 and NL = 513 cannot occur, so nobody needs to look for them: 2 S is m when m is even and m + 1 when it is odd, which makes
# NL even except when A + Lk is even (with or without the instance column), and then NL = 2 (A + Lk) + 4 Lk + 3 = 3 (mod 4), while
# 257 and 513 are 1 (mod 4).
#   (A, Lk, n_instance, k, bf, n_public)
CASES = (
    Shape(1, 1, 0, 4, 0),            # the smallest: NL = 11, M0 = 10; m = 3 odd, the last chunk is the constants alone
    Shape(1, 1, 1, 14, 5, 1025),     # m = 4: the instance column shares the last chunk with the constants; 1025 public values
    Shape(1, 1, 1, 12, 0, 1),
    Shape(2, 1, 0, 24, 5),           # NL = 12; m = 4 even, no instance column
    Shape(2, 1, 0, 4, 13),           # the largest blinding_factors with an opening: w^-(bf+1) = w^2
    Shape(123, 1, 0, 14, 5),         # NL = 255
    Shape(124, 1, 0, 4, 0),          # NL = 256 and M0 = 256
    Shape(122, 2, 0, 24, 5),         # M0 = 255
    Shape(123, 2, 0, 4, 13),         # M0 = 257
    Shape(255, 1, 0, 14, 0),         # the advice set has 255 members
    Shape(256, 2, 1, 12, 5, 1),      # 256 members; m = 260 even: constants and instance column in one chunk
    Shape(257, 3, 0, 24, 0),         # 257 members
    Shape(252, 1, 0, 14, 5),         # NL = 512
    Shape(300, 5, 1, 14, 5, 1025),   # NL = 634; m = 307 odd: the instance column alone in the last chunk
)
# blinding_factors = 2^k - 2, which pz_vk_create admits: no opening exists (Shape.degenerate), so no proof may be accepted
DEGENERATE_CASES = (Shape(2, 1, 0, 4, 14), Shape(123, 2, 0, 4, 14))
# where the three proofs of a case carry 0, 1 and r - 1 in every evaluation family / identity commitments
SPECIALS_CASES = (Shape(1, 1, 1, 12, 0, 1), Shape(252, 1, 0, 14, 5))
IDENTITY_CASES = (Shape(2, 1, 0, 24, 5), Shape(123, 1, 0, 14, 5))
IDENTITIES = (("advice", 0), ("perm_z", 0), ("h", 1), ("w1", 0))


def case_id(sh: Shape) -> str:
    return "A%d-Lk%d-i%d-k%d-bf%d-np%d" % (sh.A, sh.Lk, sh.n_instance, sh.k, sh.bf, sh.n_public)


def forge_case(sh: Shape, rng, s_tox: int, points: Callable, n_proofs: int = 3):
    """the proofs of one case: one key, distinct seeds of which one is empty, the case's specials and identities"""
    key = forge_key(sh, rng, points)
    seeds = [b"", b"forge-1"] + [b"forge-%d" % i * (i % 3 + 1) for i in range(2, n_proofs)]
    out = []
    for i in range(n_proofs):
        out.append(forge(sh, rng, seeds[i], s_tox, points, key=key, specials=i % 3 if sh in SPECIALS_CASES else None,
                         identities=IDENTITIES if sh in IDENTITY_CASES and i == 1 else ()))
    return key, seeds[:n_proofs], out
