"""GPU: decryption by the CRT (pz_paillier_sk_create_crt, pz_paillier_sk_has_crt, pz_paillier_decrypt_crt[_dev]; DESIGN.md section
15.22): the handle, the results against pz_paillier_decrypt on the SAME handle array for array and against the Python restatement
(tests/decrypt_crt_ref.py, tests/decrypt_ref.py), the structured catalogue, non-units and statuses, and the pipeline tally ->
CRT decryption -> a kind-5 proof.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyref as P
from tests import decrypt_crt_ref as CR
from tests import decrypt_ref as DR

pytestmark = pytest.mark.gpu


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


def _sk(eng, bits, standard_g, swap=False):
    k = DR.key(bits, standard_g)
    p, q = DR.primes(bits)
    if swap:
        p, q = q, p
    return eng.paillier_sk(_words(bits), k[0], k[1], k[2], k[3], p, q), k


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


def _same(a, b):
    """(m, r, flags) triples, array for array"""
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ 1. the handle
@pytest.mark.parametrize("bits,standard_g", [(128, True), (128, False), (264, True), (264, False), (2048, False), (2112, False)])
def test_crt_handle_keeps_the_lambda_path(eng, bits, standard_g):
    sk, k = _sk(eng, bits, standard_g)
    try:
        assert sk.has_crt is True
        assert sk.params() == (k[4], k[5])
    finally:
        sk.free()
    assert sk.has_crt is False      # a freed handle is forgotten


@pytest.mark.parametrize("bits", (128, 264))
def test_swapped_primes_decrypt_alike(eng, cref, bits):
    Ln = _words(bits)
    a, k = _sk(eng, bits, False)
    b, _ = _sk(eng, bits, False, swap=True)
    try:
        ms, rs, cs = DR.encryptions(k, 5, 0xc47a + bits)
        cts = np.stack([cref.int_to_limbs(c, 2 * Ln) for c in cs])
        ra, rb = eng.paillier_decrypt(a, cts, crt=True), eng.paillier_decrypt(b, cts, crt=True)
        assert _same(ra, rb) and _ints(cref, ra[0]) == ms and _ints(cref, ra[1]) == rs and ra[2].tolist() == [0] * 5
    finally:
        a.free()
        b.free()


def test_crt_handle_refusals(eng, cref):
    from paillier_halo2_amd import _lib

    for bits in (128, 264):
        Ln = _words(bits)
        n, g, lam, d, mu, ginv = DR.key(bits, standard_g=False)
        p, q = DR.primes(bits)
        mk = lambda *a: eng.paillier_sk(Ln, n, g, lam, d, *a)
        assert _status(lambda: mk(p + 2, q)) == _lib.PZ_ERR_INVALID
        assert _status(lambda: mk(p, q + 2)) == _lib.PZ_ERR_INVALID
        assert _status(lambda: mk(p + 1, q)) == _lib.PZ_ERR_INVALID          # even
        assert _status(lambda: mk(p, 2 * (q // 2))) == _lib.PZ_ERR_INVALID
        assert _status(lambda: mk(1, n)) == _lib.PZ_ERR_INVALID
        assert _status(lambda: mk(n, 1)) == _lib.PZ_ERR_INVALID
        with pytest.raises(ValueError):
            mk(p)
        with pytest.raises(ValueError):
            eng.paillier_sk(Ln, n, g, lam, d, q=q)
        # what pz_paillier_sk_create refuses is refused here through the same code
        assert _status(lambda: eng.paillier_sk(Ln, n, g, lam + 1, d, p, q)) == _lib.PZ_ERR_INVALID
        # a null prime
        w = [np.array(cref.int_to_limbs(v, Ln), dtype=np.uint64) for v in (n, g, lam, d, p, q)]
        out = _lib.VP()
        ptr = [x.ctypes.data for x in w]
        assert eng.L.pz_paillier_sk_create_crt(eng.ctx, Ln, *ptr[:5], None, C.byref(out)) == _lib.PZ_ERR_INVALID
        assert eng.L.pz_paillier_sk_create_crt(eng.ctx, Ln, *ptr[:4], None, ptr[5], C.byref(out)) == _lib.PZ_ERR_INVALID
        # the context still serves an honest key
        sk = mk(p, q)
        assert sk.has_crt and sk.params() == (mu, ginv)
        sk.free()
    # a prime whose square leaves the words of n: 3 * q' with q' of 126 bits in two words
    big = (1 << 125) + 1
    z = lambda v: np.array(cref.int_to_limbs(v, 2), dtype=np.uint64)
    n_, g_, lam_, d_ = DR.key(128, True)[:4]
    out = _lib.VP()
    a = [z(v) for v in (n_, g_, lam_, d_, 3, big)]
    assert eng.L.pz_paillier_sk_create_crt(eng.ctx, 2, *[x.ctypes.data for x in a], C.byref(out)) == _lib.PZ_ERR_UNSUPPORTED
    assert eng.L.pz_paillier_sk_has_crt(None) == 0


def test_a_handle_without_the_primes_is_not_crt(eng, cref):
    from paillier_halo2_amd import _lib

    k = DR.key(128, False)
    sk = eng.paillier_sk(2, *k[:4])
    try:
        assert sk.has_crt is False
        ms, rs, cs = DR.encryptions(k, 2, 0xc47b)
        cts = np.stack([cref.int_to_limbs(c, 4) for c in cs])
        m_, r_, f_ = np.zeros((2, 2), dtype=np.uint64), np.zeros((2, 2), dtype=np.uint64), np.zeros(2, dtype=np.uint8)
        for fn in (eng.L.pz_paillier_decrypt_crt, eng.L.pz_paillier_decrypt_crt_dev):
            assert fn(eng.ctx, sk.handle, 2, cts.ctypes.data, m_.ctypes.data, r_.ctypes.data, f_.ctypes.data) == _lib.PZ_ERR_INVALID
        assert _status(lambda: eng.paillier_decrypt(sk, cts, crt=True)) == _lib.PZ_ERR_INVALID
        m, r, fl = eng.paillier_decrypt(sk, cts)                # crt=None on such a handle: the lambda path
        assert _ints(cref, m) == ms and _ints(cref, r) == rs
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------------------------ 2. results
DEC_CASES = [(128, 1, True), (128, 65, False), (128, 300, False), (264, 3, True), (264, 65, False), (1024, 4, False), (2048, 4, True),
             (2048, 3, False), (2112, 4, False), (3072, 2, False), (4096, 2, True)]


@pytest.mark.parametrize("bits,B,standard_g", DEC_CASES)
def test_crt_equals_the_lambda_path_and_the_reference(eng, cref, bits, B, standard_g):
    import torch

    sk, k = _sk(eng, bits, standard_g)
    n, g = k[0], k[1]
    Ln = _words(bits)
    ms, rs, cs = DR.encryptions(k, B, 0xc47 + bits + B)        # 0, 1, n - 1, random; the last made with r + n
    ck = CR.crt_key(bits, standard_g)
    for i in sorted({0, B // 2, B - 1}):
        assert CR.decrypt_crt_ref(ck, cs[i]) == (ms[i], rs[i], 0)
    lim = cref.int_to_limbs
    cts = np.stack([lim(c, 2 * Ln) for c in cs])
    try:
        m, r, fl = eng.paillier_decrypt(sk, cts, crt=True)
        assert fl.tolist() == [0] * B and _ints(cref, m) == ms and _ints(cref, r) == rs
        assert _same((m, r, fl), eng.paillier_decrypt(sk, cts, crt=False))
        assert _same((m, r, fl), eng.paillier_decrypt(sk, cts))              # crt=None on a CRT handle
        m2, none, fl2 = eng.paillier_decrypt(sk, cts, want_r=False, crt=True)
        assert none is None and np.array_equal(m2, m) and np.array_equal(fl2, fl)
        # the recovered (m, r) encrypt to c: the witness of the kind-5 circuit
        t = min(B, 3)
        rep = lambda v: np.stack([lim(v, Ln)] * t)
        c_again = eng.paillier_encrypt_uniform(Ln, 64 * Ln, rep(n), rep(g), m[B - t:], r[B - t:], want_steps=False)[0]
        assert np.array_equal(c_again, cts[B - t:])
        # the device form on device buffers prefilled with a sentinel
        d_cts = torch.from_numpy(cts.view(np.int64)).cuda()
        d_m = torch.full((B, Ln), -1, dtype=torch.int64, device="cuda")
        d_r = torch.full((B, Ln), -1, dtype=torch.int64, device="cuda")
        d_f = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
        eng.sync()
        eng.paillier_decrypt_dev(sk, B, d_cts.data_ptr(), d_m.data_ptr(), d_r.data_ptr(), d_f.data_ptr(), crt=True)
        eng.sync()
        assert np.array_equal(d_m.cpu().numpy().view(np.uint64), m) and np.array_equal(d_r.cpu().numpy().view(np.uint64), r)
        assert d_f.cpu().numpy().tolist() == [0] * B
        d_m.fill_(-1)
        d_f.fill_(77)
        eng.sync()
        eng.paillier_decrypt_dev(sk, B, d_cts.data_ptr(), d_m.data_ptr(), 0, d_f.data_ptr(), crt=True)
        eng.sync()
        assert np.array_equal(d_m.cpu().numpy().view(np.uint64), m) and d_f.cpu().numpy().tolist() == [0] * B
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------------------------ 3. the catalogue
@pytest.mark.parametrize("bits", (128, 264, 2112))
def test_structured_catalogue(eng, cref, bits):
    from paillier_halo2_amd import _lib

    sk, k = _sk(eng, bits, False)
    n = k[0]
    Ln = _words(bits)
    cat = CR.catalogue(bits, False)
    inside = [e for e in cat if e[1] < n * n]
    assert len(inside) == len(cat) - 1
    cts = np.stack([cref.int_to_limbs(e[1], 2 * Ln) for e in inside])
    want_flags = [1 if e[0] in ("p*k", "q", "0") else 0 for e in inside]
    try:
        m, r, fl = eng.paillier_decrypt(sk, cts, crt=True)
        got = list(zip(_ints(cref, m), _ints(cref, r), fl.tolist()))
        for e, g_, f in zip(inside, got, want_flags):
            assert g_ == (e[2], e[3], f), e[0]
        assert _same((m, r, fl), eng.paillier_decrypt(sk, cts, crt=False))
        # n^2 itself, on the device form: bit 1 alone, zeros, the neighbours untouched
        import torch

        both = np.stack([cts[0], cref.int_to_limbs(n * n, 2 * Ln), cts[7]])
        outs = []
        for crt in (True, False):
            d_cts = torch.from_numpy(both.view(np.int64)).cuda()
            d_m = torch.full((3, Ln), -1, dtype=torch.int64, device="cuda")
            d_r = torch.full((3, Ln), -1, dtype=torch.int64, device="cuda")
            d_f = torch.full((3,), 77, dtype=torch.uint8, device="cuda")
            eng.sync()
            eng.paillier_decrypt_dev(sk, 3, d_cts.data_ptr(), d_m.data_ptr(), d_r.data_ptr(), d_f.data_ptr(), crt=crt)
            eng.sync()
            outs.append((d_m.cpu().numpy().view(np.uint64), d_r.cpu().numpy().view(np.uint64), d_f.cpu().numpy()))
        assert _same(outs[0], outs[1]) and outs[0][2].tolist() == [0, 2, 0]
        assert _ints(cref, outs[0][0]) == [inside[0][2], 0, inside[7][2]] and _ints(cref, outs[0][1]) == [inside[0][3], 0, inside[7][3]]
        assert _status(lambda: eng.paillier_decrypt(sk, both, crt=True)) == _lib.PZ_ERR_RANGE
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------------------------ 4. non-units, statuses
@pytest.mark.parametrize("bits", (128, 264, 2112))
def test_non_units_are_flagged_alone_and_the_statuses(eng, cref, bits):
    from paillier_halo2_amd import _lib

    sk, k = _sk(eng, bits, False)
    n = k[0]
    Ln = _words(bits)
    p, q = DR.primes(bits)
    ms, rs, cs = DR.encryptions(k, 3, 0xc473 + bits)
    lim = cref.int_to_limbs
    arr = lambda vs: np.stack([lim(c, 2 * Ln) for c in vs])
    try:
        for bad in (p * 0x1234567, q * 0x7654321, 0):       # p alone, q alone, both
            vs = [cs[0], bad, cs[2]]
            m, r, fl = eng.paillier_decrypt(sk, arr(vs), crt=True)
            assert fl.tolist() == [0, 1, 0] and DR.decrypt_ref(k, bad) == (0, 0, 1)
            assert _ints(cref, m) == [ms[0], 0, ms[2]] and _ints(cref, r) == [rs[0], 0, rs[2]]
            assert _same((m, r, fl), eng.paillier_decrypt(sk, arr(vs), crt=False))
        m, r, fl = eng.paillier_decrypt(sk, arr([0, q, cs[0]]), crt=True)
        assert fl.tolist() == [1, 1, 0] and _ints(cref, m) == [0, 0, ms[0]] and _ints(cref, r) == [0, 0, rs[0]]
        # a ciphertext >= n^2, in either position: PZ_ERR_RANGE
        for at in (0, 2):
            vs = list(cs)
            vs[at] = n * n
            assert _status(lambda: eng.paillier_decrypt(sk, arr(vs), crt=True)) == _lib.PZ_ERR_RANGE
        vs = [cs[0], p * 0x1234567, cs[2]]
        c_, m_, r_, f_ = arr(vs), np.zeros((3, Ln), dtype=np.uint64), np.zeros((3, Ln), dtype=np.uint64), np.zeros(3, dtype=np.uint8)
        call = lambda count: eng.L.pz_paillier_decrypt_crt(eng.ctx, sk.handle, count, c_.ctypes.data, m_.ctypes.data, r_.ctypes.data, f_.ctypes.data)
        assert call(0) == _lib.PZ_ERR_INVALID and call(65537) == _lib.PZ_ERR_INVALID
        assert eng.L.pz_paillier_decrypt_crt(eng.ctx, None, 3, c_.ctypes.data, m_.ctypes.data, r_.ctypes.data, f_.ctypes.data) == _lib.PZ_ERR_INVALID
        # the handle still serves an honest call
        assert call(3) == 0 and f_.tolist() == [0, 1, 0] and _ints(cref, m_) == [ms[0], 0, ms[2]] and _ints(cref, r_) == [rs[0], 0, rs[2]]
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------------------------ 5. the pipeline
def test_tally_crt_decrypt_proof(eng, cref):
    """three ballots -> pz_paillier_tally -> pz_paillier_decrypt_crt -> pz_paillier_encrypt_uniform_dev on the recovered (m, r) -> K4 ->
    a kind-5 proof of (n, g, sum m_i mod n, C), verified on the device: the CRT output is a valid witness (the circuit code is
    untouched).  128-bit n, 64-bit limbs, lookup_bits 14, k = 15: tests/public_ref.py's uniform shape."""
    import random

    import torch
    from paillier_halo2_amd import prover, prover_native, srs
    from paillier_halo2_amd import verifier as PV

    BITS, W, LB, K = 128, 64, 14, 15
    R = P.FR_R
    Ln, rows = BITS // W, 1 << K
    sk, k = _sk(eng, BITS, False)
    nn, g = k[0], k[1]
    lim = cref.int_to_limbs
    made = []
    try:
        ms, rs, cs = DR.encryptions(k, 3, 0xc475)
        C_, _ = eng.paillier_tally(Ln, lim(nn, Ln), np.stack([lim(c, 2 * Ln) for c in cs]), want_steps=False)
        Ci = cref.limbs_to_int(C_)
        assert Ci == cs[0] * cs[1] * cs[2] % (nn * nn)
        m_, r_, fl = eng.paillier_decrypt(sk, C_.reshape(1, -1), crt=True)
        m, r = cref.limbs_to_int(m_[0]), cref.limbs_to_int(r_[0])
        assert fl.tolist() == [0] and m == sum(ms) % nn and (m, r, 0) == DR.decrypt_ref(k, Ci) == CR.decrypt_crt_ref(CR.crt_key(BITS, False), Ci)
        # the SRS (a known toxic scalar), the native structure of kind "decrypt" with the instance column, both keys
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        s_tox = random.Random(0xc476).randrange(2, R)
        d_g = torch.zeros((rows, 8), dtype=torch.int64, device="cuda")
        d_gl = torch.zeros((rows, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(K, F(s_tox), F(P.fr_omega(K)), d_g.data_ptr(), d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(s_tox))
        params = PV.VerifierParams.from_parts(d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        bl, bm = eng.load_bases_dev(d_gl.data_ptr(), rows), eng.load_bases_dev(d_g.data_ptr(), rows)
        made += [bl, bm]
        ns = prover_native.NativeStructure(eng, "decrypt", BITS, W, LB, K, exp_r=nn, expose=True)
        made.append(ns)
        key = ns.key(bl, bm, tile=8)
        made.append(key)
        vk = PV.VerifyingKey.from_structure(eng, ns, bl, tile=8)
        # K3's uniform-shape trace of the recovered (m, r), K4's columns
        cap = ns.n_steps_g + ns.n_steps_r + 1
        d_steps = torch.zeros((cap, 4, 2 * Ln), dtype=torch.int64, device="cuda")
        c_back, _, _ = eng.paillier_encrypt_uniform_dev(Ln, BITS, lim(nn, Ln), lim(g, Ln), m_[0], r_[0], d_steps.data_ptr(), cap)
        assert cref.limbs_to_int(c_back[0]) == Ci
        d_mod = torch.from_numpy(lim(nn ** 2, 2 * Ln).astype(np.int64)).cuda()
        inputs = np.concatenate([lim(nn, Ln), lim(g, Ln), lim(m, Ln), lim(r, Ln), lim(Ci, 2 * Ln)])
        cols = torch.zeros((ns.m, rows, 4), dtype=torch.int64, device="cuda")
        eng.circuit_expand_cols_dev(5, Ln, W, LB, inputs, d_steps.data_ptr(), ns.n_steps_g, ns.n_steps_r, d_mod.data_ptr(), cols.data_ptr(),
                                    cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, rows)
        eng.sync()
        good = PV.public_inputs("decrypt", nn, g, Ci, m=m, enc_bits=BITS, limb_bits=W)
        assert good == DR.statement(nn, g, m, Ci, BITS, W) == ns.gather_public(cols.data_ptr())
        seed = b"decrypt-crt"
        proof = prover_native.create_proof(key, cols.data_ptr(), prover.HashTranscript(seed), seed=5, instances=good)
        assert PV.verify_batch_native(eng, params, vk, [proof], [seed], instances=[good]) == (True, [True])
        bad = list(good)
        bad[2 * Ln] += 1                                        # the statement's m raised by one
        assert PV.verify_batch_native(eng, params, vk, [proof], [seed], instances=[bad]) == (False, [False])
    finally:
        sk.free()
        for x in reversed(made):
            x.free()
