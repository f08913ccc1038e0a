"""GPU: the device batch verifier (pz_vk_create / pz_verify_batch, csrc/pz_verify.hip + pz_verify.cpp) held to the oracle over synthetic
key shapes, without a prover: tests/verify_forge.py constructs, for any (A, Lk, n_instance, k, blinding_factors), proofs that verify
exactly when every value the verifier derives is the oracle's -- commitments [c] G of known logs, the stated h(x) the oracle's, W2
solved from the SRS scalar the tests know.  The shapes sit on the sizes where the kernels' lane partitions turn (VF.CASES).  Every
comparison is exact: verdicts, h(x) word for word, and SHPLONK's points A and B against [a] G and [b] G from the oracle's C
restatement (not the device's fixed-base kernel), for accepted AND rejected proofs.  Then what pz_verify_batch does with words no
decoder has looked at: evaluations >= r, points off the curve, coordinates that are not canonical."""
import random
import time

import numpy as np
import pytest

from oracle import pyref as P
from tests import verify_forge as VF

pytestmark = pytest.mark.gpu

R, Q = P.FR_R, P.FQ_P
S_TOX = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
BYTES_CASES = (VF.CASES[0], VF.CASES[12])       # one small and one large shape through the wire bytes
PYTHON_CASES = (VF.CASES[0], VF.CASES[2])       # the two smallest shapes (NL = 11) through the Python verifier


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    yield e
    e.close()


class World:
    """the params of the known scalar, [c] G from the device, and per case its key handle, solved proofs and unsolved twins"""

    def __init__(self, eng, cref):
        from paillier_halo2_amd import srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.g0 = cref.affine_ints_to_mont([P.G1_GEN])[0]
        g2, s_g2 = srs.setup_g2(eng, np.array(VF.mont_words(S_TOX), dtype=np.uint64))
        self.params = PV.VerifierParams.from_parts(self.g0, g2, s_g2)
        self.cases = {}

    def points(self, logs):
        if not len(logs):
            return np.zeros((0, 8), dtype=np.uint64)
        return self.eng.g1_fixed_base_mul(np.array([VF.mont_words(c) for c in logs], dtype=np.uint64))

    def expected_point(self, log):
        """[log] G by the oracle"""
        return np.asarray(self.cref.g1_normalize(self.cref.g1_mul(self.g0, int(log) % R))).reshape(8)

    def vk(self, key):
        from paillier_halo2_amd import verifier as PV

        sh = key.shape
        return PV.VerifyingKey(sh.k, sh.bf, sh.A, sh.Lk, sh.S, key.fixed, key.sigma, sh.n_instance, sh.n_public)

    def handle(self, key):
        sh = key.shape
        return self.eng.vk_create(sh.k, sh.bf, sh.A, sh.Lk, key.fixed, key.sigma, self.params.g0, self.params.g2, self.params.s_g2,
                                  sh.n_instance, sh.n_public)

    def case(self, sh):
        if sh not in self.cases:
            rng = random.Random(sum(VF.case_id(sh).encode()))
            key, seeds, proofs = VF.forge_case(sh, rng, S_TOX, self.points)
            twins = [f.twin(rng, self.points) for f in proofs]
            self.cases[sh] = dict(key=key, seeds=seeds, proofs=proofs, twins=twins, h=self.handle(key))
        return self.cases[sh]

    def run(self, c, proofs, **kw):
        inst = [f.instances for f in proofs] if c["key"].shape.n_instance else None
        return self.eng.verify_batch_dev(c["h"], np.stack([f.words() for f in proofs]), [f.seed for f in proofs], instances=inst, **kw)

    def free(self):
        for c in self.cases.values():
            c["h"].free()


@pytest.fixture(scope="module")
def world(eng, cref):
    w = World(eng, cref)
    yield w
    w.free()


def _check_h_and_ab(world, proofs, hev, ab):
    for i, f in enumerate(proofs):
        assert np.array_equal(hev[i], f.h_words()), i
        assert np.array_equal(ab[i, 0], world.expected_point(f.a)), i
        assert np.array_equal(ab[i, 1], world.expected_point(f.b)), i


@pytest.mark.parametrize("sh", VF.CASES, ids=VF.case_id)
def test_constructed_proofs_verify_on_both_paths(world, sh):
    """three solved proofs of one key (distinct seeds, one of them empty): accepted by the fold path (one MSM, one check) and by the
    per-proof path, which also returns h(x) and A, B equal to the oracle's"""
    c = world.case(sh)
    assert len(set(c["seeds"])) == 3 and b"" in c["seeds"]
    assert c["h"].proof_words == c["proofs"][0].words().shape[0]
    assert world.run(c, c["proofs"])[:2] == (True, [True] * 3)
    ok, per, hev, ab = world.run(c, c["proofs"], want_h=True, want_ab=True)
    assert (ok, per) == (True, [True] * 3)
    _check_h_and_ab(world, c["proofs"], hev, ab)


@pytest.mark.parametrize("sh", VF.CASES, ids=VF.case_id)
def test_unsolved_twins_are_rejected_with_the_right_h_and_ab(world, sh):
    """each proof's twin with a random W2: verdict False, the same h(x), A and B still the integer predictions; in a batch of
    [solved, unsolved, solved] exactly the middle proof is flagged, whichever path gives the verdicts"""
    c = world.case(sh)
    assert all(f.holds(S_TOX) and not t.holds(S_TOX) for f, t in zip(c["proofs"], c["twins"]))
    ok, per, hev, ab = world.run(c, c["twins"], want_h=True, want_ab=True)
    assert (ok, per) == (False, [False] * 3)
    _check_h_and_ab(world, c["twins"], hev, ab)
    assert world.run(c, c["twins"])[:2] == (False, [False] * 3)
    mixed = [c["proofs"][0], c["twins"][1], c["proofs"][2]]
    assert world.run(c, mixed)[:2] == (False, [True, False, True])
    ok, per, hev, ab = world.run(c, mixed, want_h=True, want_ab=True)
    assert (ok, per) == (False, [True, False, True])
    _check_h_and_ab(world, mixed, hev, ab)


@pytest.mark.parametrize("sh", VF.DEGENERATE_CASES, ids=VF.case_id)
def test_largest_blinding_factors_accept_nothing(world, sh):
    """blinding_factors = 2^k - 2, the largest pz_vk_create admits: w^-(bf+1) x is w x, the query set of the chained permutation
    products names one point twice and no interpolation exists (VF.Shape.degenerate), so NO words are a valid proof.  The verifier must
    say so (PZ_OK, every verdict False) on either path, and h(x), which l_0, l_last and the 2^k - 2 blinding rows' Lagrange values still
    define, must be the oracle's"""
    rng = random.Random(sh.A)
    key = VF.forge_key(sh, rng, world.points)
    proofs = [VF.forge(sh, rng, sd, S_TOX, world.points, key=key, solve=False) for sd in (b"", b"d1", b"d2")]
    c = dict(key=key, h=world.handle(key))
    try:
        assert world.run(c, proofs)[:2] == (False, [False] * 3)
        ok, per, hev, _ = world.run(c, proofs, want_h=True, want_ab=True)
        assert (ok, per) == (False, [False] * 3)
        for i, f in enumerate(proofs):
            assert np.array_equal(hev[i], f.h_words()), i
    finally:
        c["h"].free()
    assert world.eng.last_hip_error() == ""


@pytest.mark.parametrize("sh", BYTES_CASES, ids=VF.case_id)
def test_constructed_proofs_verify_as_wire_bytes(world, sh):
    from paillier_halo2_amd import prover
    from paillier_halo2_amd import verifier as PV

    c = world.case(sh)
    vk = world.vk(c["key"])
    enc = lambda f: PV.proof_to_bytes(world.eng, vk, prover.Proof(commitments=f.com, evals=f.ev), handle=c["h"])
    good = [enc(f) for f in c["proofs"]]
    assert all(len(b) == PV.proof_size_bytes(vk) for b in good)
    assert PV.verify_batch_bytes(world.eng, world.params, vk, good, c["seeds"], handle=c["h"]) == (True, [True] * 3)
    mixed = [good[0], enc(c["twins"][1]), good[2]]
    assert PV.verify_batch_bytes(world.eng, world.params, vk, mixed, c["seeds"], handle=c["h"]) == (False, [True, False, True])


@pytest.mark.parametrize("sh", PYTHON_CASES, ids=VF.case_id)
def test_python_verifier_gives_the_same_verdicts(world, sh):
    from paillier_halo2_amd import prover
    from paillier_halo2_amd import verifier as PV

    c = world.case(sh)
    vk = world.vk(c["key"])
    pr = lambda f: prover.Proof(commitments=f.com, evals=f.ev)
    inst = lambda fs: [f.instances for f in fs] if sh.n_instance else None
    assert PV.verify_batch(world.eng, world.params, vk, [pr(f) for f in c["proofs"]], c["seeds"], inst(c["proofs"])) == (True, [True] * 3)
    mixed = [c["proofs"][0], c["twins"][1], c["proofs"][2]]
    assert PV.verify_batch(world.eng, world.params, vk, [pr(f) for f in mixed], c["seeds"], inst(mixed)) == (False, [True, False, True])
    assert PV.verify_batch(world.eng, world.params, vk, [pr(f) for f in c["twins"]], c["seeds"], inst(c["twins"])) == (False, [False] * 3)


def test_fold_crosses_its_blocks_and_the_fallback_flags_the_last_proof(world):
    """B = 257 proofs of shape (1, 1, 0) through the fold path only: k_verify_fold mode 0 has 7 + 257 * 13 = 3348 slots, 14 blocks of
    256 lanes, and proof 256's own slots lie in the last one.  All solved: accepted by one fold.  Then proof 256 is replaced by its
    unsolved twin: the fold fails and the per-proof fallback must flag exactly index 256.
    B = 257 is kept, not reduced: on an MI355X the accepted fold took 0.09 s and the call with the fallback (257 two-column MSMs
    and 257 checks in one launch) 2.1 s; with the forging of the 257 proofs the test takes 3.6 s."""
    sh = VF.CASES[0]
    B = 257
    rng = random.Random(257)
    key = VF.forge_key(sh, rng, world.points)
    proofs = [VF.forge(sh, rng, b"many-%d" % i, S_TOX, world.points, key=key) for i in range(B)]
    c = dict(key=key, h=world.handle(key))
    try:
        t0 = time.perf_counter()
        assert world.run(c, proofs)[:2] == (True, [True] * B)
        t1 = time.perf_counter()
        proofs[B - 1] = proofs[B - 1].twin(rng, world.points)
        ok, per, _, _ = world.run(c, proofs)
        t2 = time.perf_counter()
        print("\npz_verify_batch, shape (1, 1, 0), B = %d: fold %.3f s, fold + per-proof fallback %.3f s" % (B, t1 - t0, t2 - t1))
        assert ok is False and per == [True] * (B - 1) + [False]
    finally:
        c["h"].free()


@pytest.mark.parametrize("sh", (VF.CASES[0], VF.CASES[8]), ids=VF.case_id)
def test_defects_that_cancel_do_not_pass_the_fold(world, sh):
    """two rejecting proofs whose openings miss by e and by -e: their unweighted sum satisfies the pairing check, so only weights that
    differ from proof to proof keep the fold from accepting them.  Both must be refused, the solved proof beside them accepted."""
    c = world.case(sh)
    rng = random.Random(0xE)
    e = rng.randrange(1, R)
    t0 = c["proofs"][0].twin(rng, world.points, defect=e, s_tox=S_TOX)
    t1 = c["proofs"][1].twin(rng, world.points, defect=-e, s_tox=S_TOX)
    assert (t0.a + t1.a + S_TOX * (t0.b + t1.b)) % R == 0 and not t0.holds(S_TOX) and not t1.holds(S_TOX)
    assert world.run(c, [t0, t1, c["proofs"][2]])[:2] == (False, [False, False, True])
    assert world.run(c, [t0, t1])[:2] == (False, [False, False])


# ---- hostile words through pz_verify_batch ---------------------------------------------------------------------------------------------
HOSTILE_SHAPE = VF.Shape(2, 1, 0, 4, 5)


def U(words):
    return np.array(words, dtype=np.uint64)


def _fq_ints(words8):
    inv = pow(1 << 256, -1, Q)
    return VF.words_int(words8[:4]) * inv % Q, VF.words_int(words8[4:]) * inv % Q


def _hostile_batch(world):
    """8 solved proofs of one key; proofs 1 .. 6 carry one defect each.  -> (key, clean proofs, hostile proofs)"""
    rng = random.Random(0x686F7374)
    sh = HOSTILE_SHAPE
    key = VF.forge_key(sh, rng, world.points)

    def x_plus_p(com, ev):                       # 4: advice commitment 1 with x + p in place of x, BEFORE the transcript is replayed
        w = com["advice"][1]
        w[:4] = U(VF.int_words(VF.words_int(w[:4]) + Q))

    clean = [VF.forge(sh, rng, b"hostile-%d" % i, S_TOX, world.points, key=key) for i in range(8)]
    bad = [VF.forge(sh, random.Random(100 + i), b"hostile-%d" % i, S_TOX, world.points, key=key, tamper=x_plus_p if i == 4 else None)
           for i in range(8)]
    assert all(f.holds(S_TOX) for f in clean + bad)
    bad[0], bad[7] = clean[0], clean[7]
    for f in bad[1:7]:
        f.com = {k: v.copy() for k, v in f.com.items()}
        f.ev = {k: v.copy() for k, v in f.ev.items()}
    bad[1].ev["advice"][1, 2] = U(VF.int_words(R))                         # 1: an evaluation's words are r exactly
    bad[2].ev["sigma"][0, 0] = U(VF.int_words((1 << 256) - 1))             # 2: ... are 2^256 - 1
    x, y = _fq_ints(bad[3].com["perm_z"][0])                            # 3: (x, y + 1): canonical, off the curve
    bad[3].com["perm_z"][0] = U(VF.mont_words(x, Q) + VF.mont_words((y + 1) % Q, Q))
    assert VF.words_int(bad[4].com["advice"][1][:4]) >= Q               # 4: made in the forge (the words as sent enter the transcript)
    w = bad[5].com["w2"][0]                                             # 5: y + p on W2 (W2 enters no challenge)
    w[4:] = U(VF.int_words(VF.words_int(w[4:]) + Q))
    assert VF.words_int(w[4:]) < 1 << 256
    x, y = _fq_ints(bad[6].com["lookup_z"][0])                          # 6: (0, y), y != 0
    assert y != 0
    bad[6].com["lookup_z"][0] = U([0] * 4 + VF.mont_words(y, Q))
    return key, clean, bad


def test_hostile_words_reject_their_proof_alone(world):
    """pz_verify_batch is never laxer than pz_verify_batch_bytes: an evaluation >= r, a commitment off the curve or with a coordinate
    that is not canonical (the identity (0, 0) apart) gives verdict 0 for its proof alone, the call is PZ_OK and leaves the context
    clean, with or without A and B asked for.  Proofs 4 and 5 satisfy the opening identity as group elements (x + p, y + p reduce to
    the same point; the transcript and W2 are those of the words as sent): they are refused only for not being canonical."""
    key, clean, bad = _hostile_batch(world)
    c = dict(key=key, h=world.handle(key))
    want = [i in (0, 7) for i in range(8)]
    try:
        got = [world.run(c, bad)[:2], world.run(c, bad, want_h=True, want_ab=True)[:2]]
        print("\nhostile words: verdicts %s (fold first), %s (per proof)" % (got[0][1], got[1][1]))
        again = world.run(c, clean)[:2]
        ok, per, hev, ab = world.run(c, clean, want_h=True, want_ab=True)
        assert got[0] == (False, want) and got[1] == (False, want)
        for i in range(1, 7):                                           # each defect alone, next to one clean proof
            pair = [clean[0], bad[i]]
            assert world.run(c, pair)[:2] == (False, [True, False]), i
            assert world.run(c, pair, want_ab=True)[:2] == (False, [True, False]), i
        assert again == (True, [True] * 8) and (ok, per) == (True, [True] * 8)
        from paillier_halo2_amd import prover
        from paillier_halo2_amd import verifier as PV

        py = PV.verify_batch(world.eng, world.params, world.vk(key), [prover.Proof(commitments=f.com, evals=f.ev) for f in bad],
                             [f.seed for f in bad])
        assert py == (False, want)                                      # the Python verifier: the same verdicts
        _check_h_and_ab(world, clean, hev, ab)
    finally:
        c["h"].free()
    assert world.eng.last_hip_error() == ""
