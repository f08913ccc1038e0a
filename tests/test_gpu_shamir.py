"""GPU: t-of-T threshold decryption with Shamir shares -- the device modular inverse (pz_bigint_mod_inverse)
against pow(x, -1, mod), the combiner over signed Lagrange exponents (pz_paillier_combine_t) against the sign-split combination of
tests/shamir_ref.py in Python integers, its flags, its equality with the T-of-T combiner, and three of five trustees opening a tally
end to end with one of them proving its partial under circuit kind 7.  Every comparison is exact."""
import functools
import math
import random

import numpy as np
import pytest

from tests import shamir_ref as SR

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


def _lim(x, n):
    assert 0 <= x < 1 << (64 * n)
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)], dtype=np.uint64)


def _int(words):
    return sum(int(v) << (64 * i) for i, v in enumerate(np.asarray(words).tolist()))


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value


# ------------------------------------------------------------------------------------------------------------------ 1. the inverse
def _moduli(limbs, rng):
    """a random odd modulus with the top bit of the top word set (at limbs = 64 and 128 x + mod overflows the capacity), all ones,
    2^(64 limbs) - 189, and 3"""
    top = 1 << (64 * limbs - 1)
    return [top | rng.getrandbits(64 * limbs - 1) | 1, (1 << (64 * limbs)) - 1, (1 << (64 * limbs)) - 189, 3]


def _xs(mod, count, rng):
    special = [1, 2 % mod, mod - 1, (mod + 1) // 2, (mod - 2) % mod, 0]
    return (special + [rng.randrange(mod) for _ in range(count)])[:count]


def _check_inverse(eng, limbs, mod, xs):
    inv, flags = eng.mod_inverse(limbs, _lim(mod, limbs), np.stack([_lim(x, limbs) for x in xs]))
    want = [SR.inverse(x, mod) for x in xs]
    assert ([_int(row) for row in inv], flags.tolist()) == ([w[0] for w in want], [w[1] for w in want])


@pytest.mark.parametrize("limbs", [1, 2, 3, 32, 63, 64, 65, 96, 128])
def test_inverse_equals_pow(eng, limbs):
    """257 values under the first modulus: 65 workgroups of four waves (the last one partly filled), finishing at different trip counts"""
    rng = random.Random(0x5b00 + limbs)
    for k, mod in enumerate(_moduli(limbs, rng)):
        _check_inverse(eng, limbs, mod, _xs(mod, 257 if k == 0 else 9, rng))


def test_inverse_trip_counts_differ_within_a_workgroup(eng):
    """neighbouring waves with operands of very different lengths (1, 2^k, random full-length values) under a 4096-bit modulus"""
    limbs = 64
    rng = random.Random(0x5b10)
    mod = (1 << 4095) | rng.getrandbits(4095) | 1
    xs = [1 << rng.randrange(4095) if i % 3 == 0 else rng.getrandbits(rng.randrange(1, 4095)) | 1 if i % 3 == 1 else rng.randrange(mod)
          for i in range(257)]
    _check_inverse(eng, limbs, mod, xs)


@pytest.mark.parametrize("limbs", [2, 65])
def test_inverse_flags(eng, limbs):
    from paillier_halo2_amd import _lib

    rng = random.Random(0x5b20 + limbs)
    p, q = SR.SAFE_P, SR.SAFE_Q
    mod = p * q if limbs == 2 else p * q * ((1 << (64 * (limbs - 2) - 1)) | rng.getrandbits(64 * (limbs - 2) - 2) | 1)
    assert mod % 2 == 1 and mod.bit_length() > 64 * (limbs - 1)
    xs = [rng.randrange(1, mod) for _ in range(9)]
    xs[3], xs[5], xs[7] = p, 0, q * 3
    inv, flags = eng.mod_inverse(limbs, _lim(mod, limbs), np.stack([_lim(x, limbs) for x in xs]))
    want = [SR.inverse(x, mod) for x in xs]
    assert [w[1] for w in want][3:8:2] == [1, 1, 1]
    assert ([_int(row) for row in inv], flags.tolist()) == ([w[0] for w in want], [w[1] for w in want])
    # x = mod and x > mod: bit 1, PZ_ERR_RANGE from the host form, every other entry written
    over = list(xs)
    over[0], over[8] = mod, min(mod + 2, (1 << (64 * limbs)) - 1)
    e = _status(lambda: eng.mod_inverse(limbs, _lim(mod, limbs), np.stack([_lim(x, limbs) for x in over])))
    want = [SR.inverse(x, mod) for x in over]
    assert e.status == _lib.PZ_ERR_RANGE and [w[1] for w in want][0:9:8] == [2, 2]
    assert ([_int(row) for row in e.inv], e.flags.tolist()) == ([w[0] for w in want], [w[1] for w in want])


def test_inverse_device_form_and_refusals(eng):
    import torch
    from paillier_halo2_amd import _lib

    limbs, count = 33, 7
    rng = random.Random(0x5b30)
    mod = rng.getrandbits(64 * limbs) | (1 << (64 * limbs - 1)) | 1
    xs = _xs(mod, count - 1, rng) + [mod]
    arr = np.stack([_lim(x, limbs) for x in xs])
    d_x = torch.from_numpy(arr.astype(np.int64)).cuda()
    d_inv = torch.full((count, limbs), -1, dtype=torch.int64, device="cuda")
    d_fl = torch.full((count,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    eng.mod_inverse_dev(limbs, _lim(mod, limbs), count, d_x.data_ptr(), d_inv.data_ptr(), d_fl.data_ptr())   # x >= mod is a flag here
    eng.sync()
    want = [SR.inverse(x, mod) for x in xs]
    assert [_int(r) for r in d_inv.cpu().numpy().view(np.uint64)] == [w[0] for w in want] and d_fl.cpu().tolist() == [w[1] for w in want]
    # refusals, all before any launch and in the documented order
    L, ctx = eng.L, eng.ctx
    m, x, o = _lim(mod, 129), arr.copy(), np.zeros((count, 129), dtype=np.uint64)
    f = np.zeros(count, dtype=np.uint8)
    p = lambda a: a.ctypes.data
    for fn in (L.pz_bigint_mod_inverse, L.pz_bigint_mod_inverse_dev):
        for args in ((ctx, limbs, 1, None, p(x), p(o), p(f)), (ctx, limbs, 1, p(m), None, p(o), p(f)), (ctx, limbs, 1, p(m), p(x), None, p(f)),
                     (ctx, limbs, 1, p(m), p(x), p(o), None), (ctx, 0, 1, p(m), p(x), p(o), p(f)), (ctx, limbs, 0, p(m), p(x), p(o), p(f)),
                     (ctx, limbs, 65537, p(m), p(x), p(o), p(f)), (ctx, 129, 0, p(m), p(x), p(o), p(f))):
            assert fn(*args) == _lib.PZ_ERR_INVALID, args
        zero, even, one = np.zeros(129, dtype=np.uint64), _lim(mod - 1, 129), _lim(1, 129)
        assert fn(ctx, 129, 1, p(zero), p(x), p(o), p(f)) == _lib.PZ_ERR_UNSUPPORTED
        assert fn(ctx, limbs, 1, p(zero), p(x), p(o), p(f)) == _lib.PZ_ERR_ZERO_MODULUS
        assert fn(ctx, limbs, 1, p(even), p(x), p(o), p(f)) == _lib.PZ_ERR_INVALID
        assert fn(ctx, limbs, 1, p(one), p(x), p(o), p(f)) == _lib.PZ_ERR_INVALID
        assert fn(ctx, 1, 1, p(one), p(x), p(o), p(f)) == _lib.PZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------------------------ 2. the combiner
def _primes(bits):
    from tests import decrypt_ref as DR

    return (SR.SAFE_P, SR.SAFE_Q) if bits == 128 else DR.primes(bits)      # ordinary primes above 128 bits: correctness needs no more


@functools.lru_cache(maxsize=None)
def _dealt(bits, T, t):
    """the reference's dealing and four ciphertexts of 0, 1, n - 1 and a random message: (n, shares, mu2, ms, cts)"""
    p, q = _primes(bits)
    rng = random.Random(0x5c00 + bits + 16 * T + t)
    n, g, shares, mu2 = SR.deal(p, q, T, t, rng.randrange)
    assert n.bit_length() == bits
    ms = [rng.randrange(n), 0, n - 1, 1]
    return n, shares, mu2, ms, [SR.encrypt(n, g, m, rng.randrange(1, n), pq=(p, q)) for m in ms]


@functools.lru_cache(maxsize=None)
def _partial(bits, T, t, i, j):
    n, shares, _, _, cts = _dealt(bits, T, t)
    return SR.partial(cts[j], shares[i - 1], n, pq=_primes(bits))


def _subsets(T, t, rng):
    """1 .. t, a random t-subset in random order, T - t + 1 .. T (t = 1: all signs positive; otherwise the signs are mixed)"""
    out = []
    for s in (list(range(1, t + 1)), rng.sample(range(1, T + 1), t), list(range(T - t + 1, T + 1))):
        if s not in out:
            out.append(s)
    return out


def _parts(bits, T, t, ids, K):
    Ln = _words(bits)
    return np.stack([np.stack([_lim(_partial(bits, T, t, i, j), 2 * Ln) for j in range(K)]) for i in ids])


KEYS = [(128, 1, 1), (128, 3, 2), (128, 5, 3), (128, 7, 7), (128, 16, 9), (264, 5, 3), (2048, 5, 3), (3072, 3, 2)]


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("bits,T,t", KEYS)
def test_combiner_equals_the_reference(eng, bits, T, t, K):
    n, shares, mu2, ms, cts = _dealt(bits, T, t)
    Ln = _words(bits)
    seen = set()
    for ids in _subsets(T, t, random.Random(0x5c10 + T + t)):
        mus = SR.lagrange(T, ids)
        seen |= {m > 0 for m in mus}
        m, flags = eng.paillier_combine_t(Ln, (n, mu2, T), ids, _parts(bits, T, t, ids, K))
        want = [SR.combine(mus, [_partial(bits, T, t, i, j) for i in ids], n, mu2) for j in range(K)]
        assert [(_int(row), int(f)) for row, f in zip(m, flags)] == want == [(x, 0) for x in ms[:K]], ids
    assert seen == ({True} if t == 1 else {True, False})


@pytest.mark.parametrize("t", [2, 129])
def test_combiner_with_the_exponents_of_256_trustees(eng, t):
    """the members T - t + 1 .. T in a shuffled order; at t = 129 their exponents take exp_words = 33 (2060 bits): long interleaved chains
    at a small modulus"""
    bits, T = 128, 256
    n, shares, mu2, ms, cts = _dealt(bits, T, t)
    ids = list(range(T - t + 1, T + 1))
    random.Random(0x5c20 + t).shuffle(ids)
    mus = SR.lagrange(T, ids)
    exps, _ = eng.shamir_lagrange(T, ids)
    assert exps.shape[1] == max(-(-abs(m).bit_length() // 64) for m in mus) == (33 if t == 129 else 27)
    m, flags = eng.paillier_combine_t(_words(bits), (n, mu2, T), ids, _parts(bits, T, t, ids, 1))
    assert SR.combine(mus, [_partial(bits, T, t, i, 0) for i in ids], n, mu2) == (ms[0], 0)
    assert (_int(m[0]), flags.tolist()) == (ms[0], [0])


def test_combiner_with_unit_exponents_is_the_t_of_t_combiner(eng):
    """S = {1 .. T}, every exponent 1, no negative sign, the T-of-T key's mu2: pz_paillier_combine's output bit for bit, a flagged entry
    included"""
    from tests import partial_ref as TR

    bits, T, K = 128, 3, 4
    p, q = _primes(bits)
    rng = random.Random(0x5c30)
    n = p * q
    theta = TR.theta_of(p, q)
    shares = TR.split(theta, n * SR.lam_of(p, q), T, rng.randrange)
    mu2 = TR.mu2_of(n, n + 1, theta)
    ms = [7, 0, n - 1, rng.randrange(n)]
    cts = [SR.encrypt(n, n + 1, m, rng.randrange(1, n)) for m in ms]
    parts = [[TR.partial(c, s, n) for c in cts] for s in shares]
    parts[1][2] = parts[0][2]                                  # entry 2 does not belong together
    Ln = _words(bits)
    arr = np.stack([np.stack([_lim(u, 2 * Ln) for u in row]) for row in parts])
    m0, f0 = eng.paillier_combine(Ln, _lim(n, Ln), _lim(mu2, Ln), arr)
    m1, f1 = np.zeros_like(m0), np.zeros_like(f0)
    ones, neg = np.ones((T, 1), dtype=np.uint64), np.zeros(T, dtype=np.uint8)
    n_w, mu_w = _lim(n, Ln), _lim(mu2, Ln)                     # (kept in names: the call takes their addresses)
    rc = eng.L.pz_paillier_combine_t(eng.ctx, Ln, K, T, n_w.ctypes.data, mu_w.ctypes.data, ones.ctypes.data, 1, neg.ctypes.data,
                                     arr.ctypes.data, m1.ctypes.data, f1.ctypes.data)
    assert rc == 0 and np.array_equal(m0, m1) and np.array_equal(f0, f1)
    assert f0.tolist() == [0, 0, 1, 0] and [_int(r) for r in m0] == [ms[0], ms[1], 0, ms[3]]


def test_combiner_flags_device_form_and_refusals(eng):
    import torch
    from paillier_halo2_amd import _lib

    bits, T, t, K = 128, 5, 3, 4
    n, shares, mu2, ms, cts = _dealt(bits, T, t)
    Ln = _words(bits)
    key = (n, mu2, T)
    ids = [2, 3, 5]
    mus = SR.lagrange(T, ids)
    assert [m > 0 for m in mus] == [True, False, True]
    us = [[_partial(bits, T, t, i, j) for j in range(K)] for i in ids]
    arr = lambda rows: np.stack([np.stack([_lim(u, 2 * Ln) for u in row]) for row in rows])
    want = lambda rows, mm=mus: [SR.combine(mm, [row[j] for row in rows], n, mu2) for j in range(len(rows[0]))]
    got = lambda m, flags: [(_int(row), int(f)) for row, f in zip(m, flags)]
    # one partial replaced by another ciphertext's: bit 0 on that entry alone
    swapped = [list(r) for r in us]
    swapped[1][2] = us[1][0]
    res = got(*eng.paillier_combine_t(Ln, key, ids, arr(swapped)))
    assert res == want(swapped) == [(ms[0], 0), (ms[1], 0), (0, 1), (ms[3], 0)]
    # one partial >= n^2: bit 1 and PZ_ERR_RANGE, the other entries written
    over = [list(r) for r in us]
    over[2][1] = n * n
    e = _status(lambda: eng.paillier_combine_t(Ln, key, ids, arr(over)))
    assert e.status == _lib.PZ_ERR_RANGE and got(e.m, e.flags) == want(over) == [(ms[0], 0), (0, 2), (ms[2], 0), (ms[3], 0)]
    # t - 1 members with their own Lagrange exponents: bit 0
    few = [2, 5]
    mus_few = SR.lagrange(T, few)
    rows = [us[0], us[2]]
    res = got(*eng.paillier_combine_t(Ln, key, few, arr(rows)))
    assert res == want(rows, mus_few) == [(0, 1)] * K
    # a forged set with B = 0 mod n (the negative-exponent partial replaced by n): bit 3
    forged = [list(r) for r in us]
    forged[1][3] = n
    res = got(*eng.paillier_combine_t(Ln, key, ids, arr(forged)))
    assert res == want(forged) and res[3][0] == 0 and res[3][1] & 8 and [r[1] for r in res[:3]] == [0, 0, 0]
    # the device form: asynchronous on the context's stream, a partial >= n^2 is a flag
    d_parts = torch.from_numpy(arr(over).astype(np.int64)).cuda()
    d_m = torch.full((K, Ln), -1, dtype=torch.int64, device="cuda")
    d_fl = torch.full((K,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    eng.paillier_combine_t_dev(Ln, key, ids, K, d_parts.data_ptr(), d_m.data_ptr(), d_fl.data_ptr())
    eng.sync()
    assert got(d_m.cpu().numpy().view(np.uint64), d_fl.cpu().numpy()) == want(over)
    # refusals, all before any launch and in pz_paillier_combine's order
    L, ctx, p = eng.L, eng.ctx, lambda a: a.ctypes.data
    n_, mu_, parts = _lim(n, 65), _lim(mu2, 65), np.zeros((3, K, 130), dtype=np.uint64)
    parts[:, :, : 2 * Ln] = arr(us)
    ex, ng = np.ones((3, 64), dtype=np.uint64), np.zeros(3, dtype=np.uint8)
    m_, f_ = np.zeros((K, 65), dtype=np.uint64), np.zeros(K, dtype=np.uint8)
    zero_n, zero_e, bad_s = np.zeros(65, dtype=np.uint64), ex.copy(), np.array([0, 2, 0], dtype=np.uint8)
    zero_e[1] = 0
    ptr = lambda a: None if a is None else p(a)
    for fn in (L.pz_paillier_combine_t, L.pz_paillier_combine_t_dev):
        def call(Ln=Ln, count=K, members=3, n=n_, mu=mu_, e=ex, w=1, s=ng, u=parts, m=m_, f=f_):
            return fn(ctx, Ln, count, members, ptr(n), ptr(mu), ptr(e), w, ptr(s), ptr(u), ptr(m), ptr(f))

        for kw in (dict(n=None), dict(mu=None), dict(e=None), dict(s=None), dict(u=None), dict(m=None), dict(f=None), dict(Ln=0), dict(count=0),
                   dict(count=1025), dict(members=0), dict(members=257), dict(w=0), dict(w=65), dict(Ln=65, count=0), dict(n=zero_n, w=0)):
            assert call(**kw) == _lib.PZ_ERR_INVALID, kw
        assert call(Ln=65, n=zero_n) == _lib.PZ_ERR_UNSUPPORTED
        assert call(n=zero_n, e=zero_e) == _lib.PZ_ERR_ZERO_MODULUS
        assert call(e=zero_e, s=bad_s) == _lib.PZ_ERR_INVALID
        assert call(s=bad_s) == _lib.PZ_ERR_INVALID


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
SP1 = (128, 64, 13, 14, 1)          # tests/test_gpu_partial.py's main shape: 128-bit n, 64-bit limbs, lookup_bits 13, k = 14, K = 1


def test_three_of_five_trustees_open_a_tally_and_one_proves_its_partial(eng, cref):
    """ballots tallied with the existing entry points; trustees of a 3-of-5 key open the total with pz_paillier_partial_dev;
    trustee 3 proves circuit kind 7 with the existing structure, key, witness and prover, and the proof verifies against ITS h and not
    against another trustee's; paillier_combine_t gives the vote count, and so does another three-subset"""
    import torch
    from oracle import pyref as P
    from paillier_halo2_amd import keys, prover, prover_native, srs
    from paillier_halo2_amd import verifier as PV
    from tests import partial_ref as TR

    bits, W, lb, k, K = SP1
    rows, Ln, T, t = 1 << k, _words(bits), 5, 3
    L2 = 2 * Ln
    rng = random.Random(0x5d00)
    key, shares = keys.deal_shamir(SR.SAFE_P, SR.SAFE_Q, T, t, rand=rng.randrange)
    assert key.v_order_proved and key.n.bit_length() == bits
    n, lim = key.n, _lim
    # 1. seven voters, one candidate: the ballots and their tally
    votes = [1, 0, 1, 1, 0, 1, 1]
    ballots = [eng.paillier_ballot(Ln, lim(n, Ln), lim(key.g, Ln), np.array([v], dtype=np.uint64), np.stack([lim(rng.randrange(1, n), Ln)]), 1,
                                   want_steps=False)[0][0] for v in votes]
    total = eng.paillier_tally(Ln, lim(n, Ln), np.stack(ballots), want_steps=False)[0].reshape(1, L2)
    c = _int(total[0])
    # 2. three of the five open it; the records stay on the device
    e_bits, n_rec = 2 * bits, TR.n_records(K, 2 * bits)
    opened = {}
    for i in (1, 3, 4, 5):
        d_steps = torch.zeros((n_rec, 4, L2), dtype=torch.int64, device="cuda")
        torch.cuda.current_stream().synchronize()
        h, u = eng.paillier_partial_dev(Ln, lim(n, Ln), lim(key.v, L2), lim(shares[i - 1], L2), total, e_bits, d_steps.data_ptr(), n_rec)
        assert _int(h) == key.hs[i - 1] and _int(u[0]) == SR.partial(c, shares[i - 1], n)
        opened[i] = (u, d_steps)
    # 3. trustee 3 proves its partial: the existing kind-7 structure, key, witness expansion and prover
    s_tox = rng.randrange(2, P.FR_R)
    F = lambda x: cref.fr_ints_to_mont([x % P.FR_R])[0]
    d_g = torch.zeros((rows, 8), dtype=torch.int64, device="cuda")
    d_gl = torch.zeros((rows, 8), dtype=torch.int64, device="cuda")
    torch.cuda.current_stream().synchronize()
    eng.srs_setup_g1_dev(k, F(s_tox), F(P.fr_omega(k)), d_g.data_ptr(), d_gl.data_ptr())
    eng.sync()
    g2, s_g2 = srs.setup_g2(eng, F(s_tox))
    params = PV.VerifierParams.from_parts(d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
    bl, bm = eng.load_bases_dev(d_gl.data_ptr(), rows), eng.load_bases_dev(d_g.data_ptr(), rows)
    ns = prover_native.NativeStructure(eng, "partial", bits, W, lb, k, count=K, expose=True)
    pkey = ns.key(bl, bm, tile=8)
    try:
        vk = PV.VerifyingKey.from_structure(eng, ns, bl, tile=8)
        u3, d_steps = opened[3]
        us3 = [_int(u3[0])]
        inputs = np.concatenate([lim(n, Ln), lim(key.v, L2), lim(shares[2], L2), lim(c, L2), lim(key.hs[2], L2), lim(us3[0], L2)])
        d_mod = torch.from_numpy(lim(n * n, L2).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, rows, 4), dtype=torch.int64, device="cuda")
        torch.cuda.current_stream().synchronize()
        eng.partial_expand_cols_dev(bits // W, W, lb, K, inputs, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(),
                                    ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, rows)
        eng.sync()
        inst = PV.public_inputs("partial", n=n, v=key.v, h=key.hs[2], cts=[c], partials=us3, enc_bits=bits, limb_bits=W)
        assert ns.gather_public(cols.data_ptr()) == inst
        seed = b"shamir-trustee-3"
        proof = prover_native.create_proof(pkey, cols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=inst)
        assert proof.h_degree_ok
        other = PV.public_inputs("partial", n=n, v=key.v, h=key.hs[0], cts=[c], partials=us3, enc_bits=bits, limb_bits=W)
        assert PV.verify_batch_native(eng, params, vk, [proof, proof], [seed, seed], instances=[inst, other]) == (False, [True, False])
    finally:
        pkey.free()
        ns.free()
        bl.free()
        bm.free()
    # 4. / 5. two different three-subsets give the vote count
    for ids in ([1, 3, 4], [5, 4, 1]):
        m, flags = eng.paillier_combine_t(Ln, key, ids, np.stack([opened[i][0] for i in ids]))
        assert (flags.tolist(), _int(m[0])) == ([0], sum(votes)), ids
