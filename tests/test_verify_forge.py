"""CPU: the proof forge of the verifier's shape tests (tests/verify_forge.py) against the product's Python verifier, over the whole shape
list: the forge's challenges, h(x) and the logs a, b of SHPLONK's A and B -- all from the oracle -- are what verifier.replay_transcript,
verifier.constraint_expression and verifier._terms give, a + s b == 0 (mod r) for a solved proof and not for its unsolved twin."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import verify_forge as VF

R = P.FR_R
S_TOX = 0x1F0A3C55AA7713B9D2C4E6F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3 % R


@pytest.fixture(scope="module")
def points(cref):
    """[c] G by the oracle's C restatement"""
    g = cref.affine_ints_to_mont([P.G1_GEN])[0]

    def fn(logs):
        return np.stack([cref.g1_normalize(cref.g1_mul(g, int(c) % R)) for c in logs]) if len(logs) else np.zeros((0, 8), dtype=np.uint64)

    return fn


def _python_terms(f):
    """h(x), challenges and the logs of A and B as the product's Python verifier forms them for the forged proof"""
    from paillier_halo2_amd import verifier as PV

    sh, key = f.shape, f.key
    vk = PV.VerifyingKey(sh.k, sh.bf, sh.A, sh.Lk, sh.S, key.fixed, key.sigma, sh.n_instance, sh.n_public)
    ch = PV.replay_transcript(f.seed, f.com, f.ev, f.instances)
    e = {fam: rows for fam, rows in f.evi.items() if fam not in ("constants", "h")}
    x = ch["x"]
    inst_x = PV.instance_eval(sh.k, f.instances, x) if sh.n_instance else None
    h = PV.constraint_expression(vk, e, ch["beta"], ch["gamma"], ch["y"], x, inst_x) * pow(pow(x, 1 << sh.k, R) - 1, -1, R) % R
    if sh.degenerate():
        return ch, h, None, None, None
    t = PV._terms(vk, f.com, f.ev, f.seed, f.instances)
    log_of = {}
    for fam, logs in f.clog.items():
        for c, w in zip(logs, f.com[fam]):
            log_of[np.asarray(w, dtype=np.uint64).tobytes()] = c
    lg = [log_of[np.asarray(b, dtype=np.uint64).tobytes()] for b in t.bases]
    a = (sum(int(sc) * c for sc, c in zip(t.vk_scalars, key.fixed_log + key.sigma_log)) + t.g_scalar +
         sum(int(sc) * c for sc, c in zip(t.a_scalars, lg))) % R
    b = sum(int(sc) * c for sc, c in zip(t.b_scalars, lg)) % R
    return ch, h, t.ok, a, b


@pytest.mark.parametrize("sh", VF.CASES, ids=VF.case_id)
def test_forge_agrees_with_the_python_verifier(sh, points):
    rng = random.Random(sum(VF.case_id(sh).encode()))
    key, seeds, proofs = VF.forge_case(sh, rng, S_TOX, points)
    assert len(set(seeds)) == 3 and b"" in seeds
    for f in proofs:
        for g in (f, f.twin(rng, points)):
            ch, h, ok, a, b = _python_terms(g)
            assert ch == g.ch and h == g.h and ok is True
            assert (a, b) == (g.a, g.b)
            assert g.holds(S_TOX) is g.solved
        assert f.words().shape == (8 * sh.n_own + 4 * sum(n * q for n, q in sh.eval_shapes().values()),)
    if sh in VF.SPECIALS_CASES:
        for fam in VF.EVAL_ORDER[:-1]:
            seen = {v for f in proofs for row in f.evi[fam] for v in row}
            assert set(VF.SPECIAL_VALUES) <= seen, fam
    if sh in VF.IDENTITY_CASES:
        assert all(not proofs[1].com[fam][i].any() for fam, i in VF.IDENTITIES)


def test_case_list_covers_what_it_claims():
    """the sizes the lane partitions turn on, both parities of m with the instance column, every k and blinding_factors with a small
    and a large shape"""
    nl = {sh.NL for sh in VF.CASES}
    m0 = {sh.M0 for sh in VF.CASES}
    adv = {sh.A for sh in VF.CASES}
    assert {11, 12, 255, 256, 512, 634} <= nl and {255, 256, 257} <= m0 and {255, 256, 257} <= adv
    assert {sh.m % 2 for sh in VF.CASES if sh.n_instance} == {0, 1}
    assert {sh.n_public for sh in VF.CASES if sh.n_instance} == {1, 1025} and all(sh.k >= 12 for sh in VF.CASES if sh.n_instance)
    for small in (True, False):
        group = [sh for sh in VF.CASES + VF.DEGENERATE_CASES if (sh.A <= 2) is small]
        assert {4, 14, 24} <= {sh.k for sh in group}
        assert {0, 5, 13, 14} <= {sh.bf for sh in group}
    assert all(sh.degenerate() and sh.k == 4 for sh in VF.DEGENERATE_CASES) and not any(sh.degenerate() for sh in VF.CASES)


@pytest.mark.parametrize("sh", VF.DEGENERATE_CASES, ids=VF.case_id)
def test_no_opening_exists_at_the_largest_blinding_factors(sh, points):
    """blinding_factors = 2^k - 2: w^-(bf+1) x IS w x, the oracle has no interpolation over a repeated point, and the forge says so;
    h(x) and the challenges are still defined and agree with the Python verifier's"""
    rng = random.Random(14)
    pts = sh.rotation_points(12345)
    assert pts[4] == pts[1]
    with pytest.raises(ValueError):
        VF.forge(sh, rng, b"x", S_TOX, points)
    f = VF.forge(sh, rng, b"x", S_TOX, points, solve=False)
    ch, h, _, _, _ = _python_terms(f)
    assert ch == f.ch and h == f.h and f.a is None and f.b is None


def test_twins_with_a_chosen_defect(points):
    """the twin whose opening misses by a stated amount: two of them with defects e and -e cancel in an unweighted sum"""
    rng = random.Random(99)
    sh = VF.CASES[0]
    key, _, (f0, f1, _) = VF.forge_case(sh, rng, S_TOX, points)
    e = rng.randrange(1, R)
    t0, t1 = f0.twin(rng, points, defect=e, s_tox=S_TOX), f1.twin(rng, points, defect=-e, s_tox=S_TOX)
    assert (t0.a + S_TOX * t0.b) % R == e and (t1.a + S_TOX * t1.b) % R == R - e
    assert not t0.holds(S_TOX) and not t1.holds(S_TOX) and (t0.a + t1.a + S_TOX * (t0.b + t1.b)) % R == 0
    for g in (t0, t1):
        _, _, ok, a, b = _python_terms(g)
        assert ok is True and (a, b) == (g.a, g.b)
