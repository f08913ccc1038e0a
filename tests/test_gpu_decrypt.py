"""GPU: decryption with randomness recovery (pz_paillier_sk_*, pz_paillier_decrypt[_dev]) and the decrypt circuit (kind 5 / "decrypt";
DESIGN.md section 15.9) through every layer -- the key handle, the batched decryption (K3), the cell stream (K4), the native structure
generator, and the pipeline tally -> decrypt -> proof of "C decrypts to m" by both provers -- against the restatement of
tests/decrypt_ref.py in Python integers.  Every comparison is exact.

Circuit shape: 128-bit n, 64-bit limbs, lookup_bits 14, k = 15 -- tests/public_ref.py's uniform shape."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import decrypt_ref as DR
from tests import public_ref as PR

pytestmark = pytest.mark.gpu

R = P.FR_R
BF = 6
BITS, W, LB, K = 128, 64, 14, 15


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _words(bits):
    return -(-bits // 64)


def _ints(cref, a):
    return [cref.limbs_to_int(row) for row in a]


def _sk(eng, k, bits):
    n, g, lam, d = k[:4]
    return eng.paillier_sk(_words(bits), n, g, lam, d)


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


# ------------------------------------------------------------------------------------------------------------------ 1. the key handle
# Ln = 2; Ln = 5 (n does not fill its top word); 1024; L = 64, the last one-limb-per-lane size; L = 66, the first two-limb one; L = 96;
# L = 128, the largest
@pytest.mark.parametrize("bits", DR.KEY_BITS)
@pytest.mark.parametrize("standard_g", [True, False], ids=["g=n+1", "general-g"])
def test_key_handle_derives_mu_and_ginv(eng, bits, standard_g):
    k = DR.key(bits, standard_g)
    sk = _sk(eng, k, bits)
    try:
        assert sk.params() == (k[4], k[5])
        assert (k[5] == 1) == standard_g      # g = n + 1 is 1 mod n: the decryption skips its ginv^m chain there, and only there
    finally:
        sk.free()
    sk.free()       # a freed handle is forgotten: a second free is a no-op


def test_key_handle_refusals(eng, cref):
    from paillier_halo2_amd import _lib

    for bits in (128, 264):
        Ln = _words(bits)
        n, g, lam, d, mu, ginv = DR.key(bits, standard_g=False)
        mk = lambda *a: eng.paillier_sk(Ln, *a)
        assert _status(lambda: mk(n, g, lam + 1, d)) == _lib.PZ_ERR_INVALID
        assert _status(lambda: mk(n, g, lam, d + 1)) == _lib.PZ_ERR_INVALID
        assert _status(lambda: mk(n, 1, lam, d)) == _lib.PZ_ERR_INVALID
        assert _status(lambda: mk(n, g, 0, d)) == _lib.PZ_ERR_INVALID
        assert _status(lambda: mk(n, g, n, d)) == _lib.PZ_ERR_INVALID            # lambda must lie below n
        assert _status(lambda: mk(0, g, lam, d)) == _lib.PZ_ERR_ZERO_MODULUS
        # the context still serves an honest key
        sk = mk(n, g, lam, d)
        assert sk.params() == (mu, ginv)
        sk.free()
    z = np.zeros(65, dtype=np.uint64)
    z[0] = 5
    out = _lib.VP()
    import ctypes as C

    assert eng.L.pz_paillier_sk_create(eng.ctx, 65, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, C.byref(out)) == _lib.PZ_ERR_UNSUPPORTED
    assert eng.L.pz_paillier_sk_create(eng.ctx, 0, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, C.byref(out)) == _lib.PZ_ERR_INVALID
    assert eng.L.pz_paillier_sk_free(eng.ctx, None) == 0


# ------------------------------------------------------------------------------------------------------------------ 2. decrypt
DEC_CASES = [(128, 1, True), (128, 3, False), (128, 65, False), (128, 300, True), (264, 1, False), (264, 3, True), (264, 65, True),
             (264, 300, False), (1024, 4, False), (2048, 4, True), (2048, 3, False), (2112, 4, False), (3072, 2, False), (4096, 2, True)]


@pytest.mark.parametrize("bits,B,standard_g", DEC_CASES)
def test_decrypt_equals_the_reference_bit_for_bit(eng, cref, bits, B, standard_g):
    import torch

    k = DR.key(bits, standard_g)
    n, g = k[0], k[1]
    Ln = _words(bits)
    ms, rs, cs = DR.encryptions(k, B, 0xdec2 + bits + B)        # 0, 1, n - 1, random; the last made with r + n
    lim = cref.int_to_limbs
    cts = np.stack([lim(c, 2 * Ln) for c in cs])
    sk = _sk(eng, k, bits)
    try:
        m, r, fl = eng.paillier_decrypt(sk, cts)
        assert fl.tolist() == [0] * B and _ints(cref, m) == ms and _ints(cref, r) == rs
        m2, none, fl2 = eng.paillier_decrypt(sk, cts, want_r=False)
        assert none is None and np.array_equal(m2, m) and np.array_equal(fl2, fl)
        # the recovered (m, r) encrypt to c: the witness of the kind-5 circuit
        t = min(B, 3)
        rep = lambda v: np.stack([lim(v, Ln)] * t)
        c_again = eng.paillier_encrypt_uniform(Ln, 64 * Ln, rep(n), rep(g), m[B - t:], r[B - t:], want_steps=False)[0]
        assert np.array_equal(c_again, cts[B - t:])
        # the device form on device buffers
        d_cts = torch.from_numpy(cts.view(np.int64)).cuda()
        d_m = torch.full((B, Ln), -1, dtype=torch.int64, device="cuda")
        d_r = torch.full((B, Ln), -1, dtype=torch.int64, device="cuda")
        d_f = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
        eng.sync()
        eng.paillier_decrypt_dev(sk, B, d_cts.data_ptr(), d_m.data_ptr(), d_r.data_ptr(), d_f.data_ptr())
        eng.sync()
        assert np.array_equal(d_m.cpu().numpy().view(np.uint64), m) and np.array_equal(d_r.cpu().numpy().view(np.uint64), r)
        assert d_f.cpu().numpy().tolist() == [0] * B
    finally:
        sk.free()


@pytest.mark.parametrize("bits", (128, 264, 2112))
def test_a_non_unit_is_flagged_alone_and_the_statuses(eng, cref, bits):
    from paillier_halo2_amd import _lib

    k = DR.key(bits, standard_g=False)
    n = k[0]
    Ln = _words(bits)
    p, q = DR.primes(bits)
    ms, rs, cs = DR.encryptions(k, 3, 0xdec3 + bits)
    cs[1] = p * 0x1234567
    lim = cref.int_to_limbs
    arr = lambda vs: np.stack([lim(c, 2 * Ln) for c in vs])
    sk = _sk(eng, k, bits)
    try:
        m, r, fl = eng.paillier_decrypt(sk, arr(cs))
        assert fl.tolist() == [0, 1, 0] and DR.decrypt_ref(k, cs[1]) == (0, 0, 1)
        assert _ints(cref, m) == [ms[0], 0, ms[2]] and _ints(cref, r) == [rs[0], 0, rs[2]]
        m, r, fl = eng.paillier_decrypt(sk, arr([0, q, cs[0]]))
        assert fl.tolist() == [1, 1, 0] and _ints(cref, m) == [0, 0, ms[0]] and _ints(cref, r) == [0, 0, rs[0]]
        # a ciphertext >= n^2, in either position: PZ_ERR_RANGE
        for at in (0, 2):
            vs = list(cs)
            vs[at] = n * n
            assert _status(lambda: eng.paillier_decrypt(sk, arr(vs))) == _lib.PZ_ERR_RANGE
        c_, m_, r_, f_ = arr(cs), np.zeros((3, Ln), dtype=np.uint64), np.zeros((3, Ln), dtype=np.uint64), np.zeros(3, dtype=np.uint8)
        call = lambda count: eng.L.pz_paillier_decrypt(eng.ctx, sk.handle, count, c_.ctypes.data, m_.ctypes.data, r_.ctypes.data, f_.ctypes.data)
        assert call(0) == _lib.PZ_ERR_INVALID and call(65537) == _lib.PZ_ERR_INVALID
        assert eng.L.pz_paillier_decrypt(eng.ctx, None, 3, c_.ctypes.data, m_.ctypes.data, r_.ctypes.data, f_.ctypes.data) == _lib.PZ_ERR_INVALID
        # the handle still serves an honest call
        assert call(3) == 0 and f_.tolist() == [0, 1, 0] and _ints(cref, m_) == [ms[0], 0, ms[2]]
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------------------------ 3. kind 5
class World:
    """the circuit shape under the 128-bit fixture key with a general g: SRS with a known toxic scalar, both structures of kind
    "decrypt" with the instance column, both keys, witnesses from K3 -> K4"""

    def __init__(self, eng, cref):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.Ln = Ln = BITS // W
        self.n_rows = n = 1 << K
        self.key5 = DR.key(BITS, standard_g=False)
        self.nn, self.g = self.key5[0], self.key5[1]
        self.sk = _sk(eng, self.key5, BITS)
        rng = random.Random(0xdec4)
        self.s_tox = rng.randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(K, F(self.s_tox), F(P.fr_omega(K)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        self.ns = prover_native.NativeStructure(eng, "decrypt", BITS, W, LB, K, exp_r=self.nn, expose=True)
        self.sa = CS.stream_structure("decrypt", BITS, W, LB, 0, self.nn)
        self.cs, self.starts = CS.columns(self.sa, K, LB, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)

    def records(self, m, r):
        """K3's uniform-shape trace of (n, g, m, r) on the device -> (records, its result as an integer)"""
        import torch

        cref, Ln, ns = self.cref, self.Ln, self.ns
        arr = lambda v, l: cref.int_to_limbs(v, l)
        cap = ns.n_steps_g + ns.n_steps_r + 1
        d_steps = torch.zeros((cap, 4, 2 * Ln), dtype=torch.int64, device="cuda")
        c, _, _ = self.eng.paillier_encrypt_uniform_dev(Ln, BITS, arr(self.nn, Ln), arr(self.g, Ln), arr(m, Ln), arr(r, Ln), d_steps.data_ptr(), cap)
        return d_steps, cref.limbs_to_int(c[0])

    def expand(self, kind_id, m, r, res, d_steps, dense=False):
        """K4's cells of circuit `kind_id` from the records: the columns [m'][2^k][4], or the dense streams"""
        import torch

        eng, cref, Ln, ns = self.eng, self.cref, self.Ln, self.ns
        arr = lambda v, l: cref.int_to_limbs(v, l)
        d_mod = torch.from_numpy(arr(self.nn ** 2, 2 * Ln).astype(np.int64)).cuda()
        inputs = np.concatenate([arr(self.nn, Ln), arr(self.g, Ln), arr(m, Ln), arr(r, Ln), arr(res, 2 * Ln)])
        if dense:
            na, nl = eng.circuit_cells(kind_id, Ln, W, LB, ns.n_steps_g, ns.n_steps_r)
            d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
            d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
            eng.circuit_expand_dev(kind_id, Ln, W, LB, inputs, d_steps.data_ptr(), ns.n_steps_g, ns.n_steps_r, d_mod.data_ptr(), d_adv.data_ptr(),
                                   d_lk.data_ptr())
            eng.sync()
            return d_adv, d_lk
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        eng.circuit_expand_cols_dev(kind_id, Ln, W, LB, inputs, d_steps.data_ptr(), ns.n_steps_g, ns.n_steps_r, d_mod.data_ptr(), cols.data_ptr(),
                                    cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, self.n_rows)
        eng.sync()
        return cols

    def witness(self, m, r):
        d_steps, c = self.records(m, r)
        return self.expand(5, m, r, c, d_steps), c

    def close(self):
        self.sk.free()
        self.key.free()
        self.ns.free()
        self.bl.free()
        self.bm.free()


@pytest.fixture(scope="module")
def world(eng, cref):
    w = World(eng, cref)
    yield w
    w.close()


def test_kind5_cells_are_kind2s_byte_for_byte(eng, cref, world):
    import torch

    w = world
    ms, rs, cs = DR.encryptions(w.key5, 2, 0xdec5)
    m, r, c = ms[1], rs[1], cs[1]
    d_steps, c_dev = w.records(m, r)
    assert c_dev == c
    assert eng.circuit_cells(5, w.Ln, W, LB, w.ns.n_steps_g, w.ns.n_steps_r) == eng.circuit_cells(2, w.Ln, W, LB, w.ns.n_steps_g, w.ns.n_steps_r)
    a5, l5 = w.expand(5, m, r, c, d_steps, dense=True)
    a2, l2 = w.expand(2, m, r, c, d_steps, dense=True)
    assert torch.equal(a5, a2) and torch.equal(l5, l2) and bool(a5.any())
    want_cells, want_adv = DR.exposed_cells(w.nn, w.g, m, r, c, BITS, W, LB)
    assert cref.fr_mont_to_ints(a5.cpu().numpy().view(np.uint64)) == want_adv
    cols5, cols2 = w.expand(5, m, r, c, d_steps), w.expand(2, m, r, c, d_steps)
    assert torch.equal(cols5, cols2)
    # the statement gathered from the columns
    assert w.ns.gather_public(cols5.data_ptr()) == DR.statement(w.nn, w.g, m, c, BITS, W)


def test_native_structure_equals_the_python_generator(eng, cref, world):
    import ctypes as C
    from paillier_halo2_amd import prover_native

    w = world
    ns, cs, sa = w.ns, w.cs, w.sa
    Ln = w.Ln
    assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
    assert (ns.n_cells, ns.n_lookups, ns.n_steps_g) == (sa.n_cells, sa.lookup_src.shape[0], 2 * BITS) and ns.n_steps_r == sa.n_steps_r
    assert ns.starts().tolist() == w.starts.tolist() and ns.constants() == [int(c) for c in cs.constants]
    sel, mc, mr = ns.download()
    assert np.array_equal(sel, cs.selectors)
    assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
    assert (ns.n_instance, ns.n_public) == (1, 5 * Ln) and ns.public_cells() == cs.public_cells
    # pz_circuit_public_cells(5) is the restatement's list
    ms, rs, cs_ = DR.encryptions(w.key5, 1, 0xdec6)
    want_cells, _ = DR.exposed_cells(w.nn, w.g, ms[0], rs[0], cs_[0], BITS, W, LB)
    out, npub = np.zeros(5 * Ln, dtype=np.uint64), C.c_size_t()
    assert eng.L.pz_circuit_public_cells(5, Ln, W, LB, ns.n_steps_g, ns.n_steps_r, out.ctypes.data, 5 * Ln, C.byref(npub)) == 0
    assert out.tolist() == want_cells == sa.public_cells.tolist()
    # kind 2's structure: the same arrays but for the instance column's ties
    u = prover_native.NativeStructure(eng, "encrypt_uniform", BITS, W, LB, K, exp_r=w.nn, expose=True)
    try:
        sel2, mc2, mr2 = u.download()
        assert np.array_equal(sel, sel2) and u.starts().tolist() == ns.starts().tolist() and u.constants() == ns.constants()
        assert (u.n_public, u.m) == (4 * Ln, ns.m) and u.public_cells() == ns.public_cells()[:2 * Ln] + ns.public_cells()[3 * Ln:]
    finally:
        u.free()


def _oracle_checks(cref, w, pr, seed, inst):
    """oracle/verifier.py's checks with the statement in the transcript: the identity at x from the evaluations, SHPLONK's final identity"""
    from oracle import verifier as V
    from paillier_halo2_amd import prover

    A, Lk, m = w.ns.n_adv, w.ns.n_lk, w.ns.m
    S = -(-m // 2)
    ev = {f: PR.ints_of(cref, v) for f, v in pr.evals.items()}
    ch = PR.replay_challenges_pub(seed, inst, pr.commitments, pr.evals)
    inst_x = PR.instance_eval(K, inst, ch["x"])
    ident = PR.expected_h_pub(K, BF, A, Lk, prover.CHUNK, ev, ch["beta"], ch["gamma"], ch["y"], ch["x"], prover.DELTA, inst_x) == ev["h"][0][0]
    xn = pow(ch["x"], w.n_rows, R)
    hc = cref.g1_normalize(cref.msm_g1(cref.fr_ints_to_mont([pow(xn, i, R) for i in range(3)]), pr.commitments["h"]))
    vk_c = w.key.vk_commitments()
    com = dict(pr.commitments)
    com.update(fixed=vk_c["fixed"], sigma=vk_c["sigma"], h=[hc])
    opening = V.shplonk_check(cref, PR.query_layout_pub(A, Lk, m, S), prover.rotation_points(w.pk.dom, ch["x"]), com, ev, ch["sh_y"], ch["sh_v"],
                              ch["sh_u"], pr.commitments["w1"][0], pr.commitments["w2"][0], w.s_tox)
    return pr.h_degree_ok, ident, opening


def test_pipeline_tally_decrypt_prove_and_the_negatives(eng, cref, world):
    """three ballots -> pz_paillier_tally -> pz_paillier_decrypt -> a kind-5 proof of (n, g, sum m_i mod n, C) by both provers; a second
    ciphertext under the same key; the wire; then each way of lying is rejected"""
    from paillier_halo2_amd import _lib, prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    Ln, nn, g = w.Ln, w.nn, w.g
    lim = cref.int_to_limbs
    ms, rs, cs = DR.encryptions(w.key5, 3, 0xdec7)
    C_, _ = eng.paillier_tally(Ln, lim(nn, Ln), np.stack([lim(c, 2 * Ln) for c in cs]), want_steps=False)
    Ci = cref.limbs_to_int(C_)
    assert Ci == cs[0] * cs[1] * cs[2] % (nn * nn)
    m_, r_, fl = eng.paillier_decrypt(w.sk, C_.reshape(1, -1))
    m, r = cref.limbs_to_int(m_[0]), cref.limbs_to_int(r_[0])
    assert fl.tolist() == [0] and m == sum(ms) % nn and (m, r, 0) == DR.decrypt_ref(w.key5, Ci)
    good = PV.public_inputs("decrypt", nn, g, Ci, m=m, enc_bits=BITS, limb_bits=W)
    assert good == DR.statement(nn, g, m, Ci, BITS, W) and len(good) == 5 * Ln
    cols, c_wit = w.witness(m, r)
    assert c_wit == Ci and w.ns.gather_public(cols.data_ptr()) == good
    # a second ciphertext under the same key: the first ballot on its own
    m2_, r2_, _ = eng.paillier_decrypt(w.sk, lim(cs[0], 2 * Ln).reshape(1, -1))
    m2, r2 = cref.limbs_to_int(m2_[0]), cref.limbs_to_int(r2_[0])
    other = PV.public_inputs("decrypt", nn, g, cs[0], m=m2, enc_bits=BITS, limb_bits=W)
    cols2, _ = w.witness(m2, r2)
    assert (m2, r2) == (ms[0], rs[0]) and w.ns.gather_public(cols2.data_ptr()) == other != good
    seeds = [b"decrypt-stepper", b"decrypt-python", b"decrypt-second"]
    p0 = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seeds[0]), seed=5, instances=good)
    p1 = prover.create_proof(w.pk, w.witness(m, r)[0], prover.HashTranscript(seeds[1]), seed=6, tile=8, instances=good)
    p2 = prover_native.create_proof(w.key, cols2.data_ptr(), prover.HashTranscript(seeds[2]), seed=7, instances=other)
    proofs, inst = [p0, p1, p2], [good, good, other]
    for pr, seed, st in zip(proofs, seeds, inst):
        assert _oracle_checks(cref, w, pr, seed, st) == (True, True, True)
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])      # pz_verify_batch_pub
    assert PV.verify_batch(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])
    wire = [PV.proof_to_bytes(eng, w.vk, p) for p in proofs]
    assert PV.verify_batch_bytes(eng, w.params, w.vk, wire, seeds, instances=inst) == (True, [True, True, True])
    assert PV.proof_to_bytes(eng, w.vk, PV.proof_from_bytes(eng, w.vk, wire[0])) == wire[0]
    # ---- negatives.  (a) the statement's m raised by one; (b) one limb of the statement's c changed
    for at in (2 * Ln, 3 * Ln + 1):
        bad = [list(s) for s in inst]
        bad[0][at] += 1
        assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=bad) == (False, [False, True, True])
        assert PV.verify_batch(eng, w.params, w.vk, proofs, seeds, instances=bad) == (False, [False, True, True])
    # (c) a witness made with r + 1: a satisfied circuit, but its result is no longer C -- the honest statement does not fit it
    r_bad = r + 1
    cols_bad, c_bad = w.witness(m, r_bad)
    assert c_bad == P.paillier_enc_native(nn, g, m, r_bad) != Ci
    sd = b"decrypt-forged"
    pf = prover_native.create_proof(w.key, cols_bad.data_ptr(), prover.HashTranscript(sd), seed=9, instances=good)
    assert not pf.h_degree_ok
    assert PV.verify_batch_native(eng, w.params, w.vk, [pf, p0], [sd, seeds[0]], instances=[good, good]) == (False, [False, True])
    pf2 = prover.create_proof(w.pk, w.witness(m, r_bad)[0], prover.HashTranscript(sd), seed=9, tile=8, instances=good)
    assert PV.verify_batch_native(eng, w.params, w.vk, [pf2], [sd], instances=[good]) == (False, [False])
    # (d) the kind-5 statement offered to a kind-2 key: its n_public is 4 Ln, PZ_ERR_INVALID
    u = prover_native.NativeStructure(eng, "encrypt_uniform", BITS, W, LB, K, exp_r=nn, expose=True)
    try:
        vk2 = PV.VerifyingKey.from_structure(eng, u, w.bl, tile=8)
        assert (vk2.n_public, w.vk.n_public) == (4 * Ln, 5 * Ln)
        h2 = PV.native_key(eng, w.params, vk2)
        try:
            words = np.stack([PV.pack_proof(vk2, p0.commitments, p0.evals)])
            assert _status(lambda: eng.verify_batch_dev(h2, words, seeds[:1], instances=[good])) == _lib.PZ_ERR_INVALID
            # ... and with the kind-2 statement n | g | c the kind-5 proof is simply false under that key
            assert eng.verify_batch_dev(h2, words, seeds[:1], instances=[good[:2 * Ln] + good[3 * Ln:]])[1] == [False]
        finally:
            h2.free()
    finally:
        u.free()
