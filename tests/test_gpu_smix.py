"""GPU: the short-randomness mix (kind 10 / "smix") -- the route layers, the hs-chains and the outputs of
pz_paillier_smix[_dev] against the independent restatement of tests/smix_ref.py in Python integers, bit for bit, and against the
kernels it is made from (pz_paillier_mix's routes, pz_paillier_partial's chain); every refusal; K4's stream, the native structure,
connected proofs of two mixes under two keys with ONE proving key, the eight forged edges, and sballots through two mixers into
decryption.  Keys: tests/golden/paillier_keys.json and oracle.pyref.synth_paillier_inputs; every seed is fixed here."""
import math
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import decrypt_ref as DR
from tests import public_ref as PR
from tests import smix_ref as XR

pytestmark = pytest.mark.gpu

R = P.FR_R
BF = 6


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _words(bits):
    return -(-bits // 64)


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


def _perm(K, seed):
    p = list(range(K))
    random.Random(seed).shuffle(p)
    return p


def _unit(rng, n):
    while True:
        x = rng.randrange(2, n)
        if math.gcd(x, n) == 1:
            return x


def _specials(s_bits):
    return [0, (1 << s_bits) - 1, 1 << (s_bits - 1)]            # zero, all ones, a lone top bit


def _inputs(bits, K, s_bits, seed, n=None):
    """sballots under the fixture key of the size (or under n); s: 0, all ones, a lone top bit, then random"""
    rng = random.Random(seed)
    n = DR.key(bits)[0] if n is None else n
    g = n + 1
    hs = XR.djn_hs(n, _unit(rng, n))
    cts = [XR.encrypt(n, g, hs, rng.randrange(1 << 16), rng.randrange(1 << min(s_bits, 64))) for _ in range(K)]
    sp = list(dict.fromkeys(_specials(s_bits)))
    # the random value first: K = 1 and K = 2 still run a chain that is neither empty nor full
    ss = [rng.randrange(1 << s_bits)] + [sp[(i - 1) % len(sp)] if i <= len(sp) else rng.randrange(1 << s_bits) for i in range(1, K)]
    return n, hs, cts, ss


def _arr(cref, values, L):
    return np.stack([cref.int_to_limbs(v, L) for v in values])


def _smix(eng, cref, bits, n, hs, cts, sw, ss, s_bits, **kw):
    Ln = _words(bits)
    lim = cref.int_to_limbs
    return eng.paillier_smix(Ln, lim(n, Ln), lim(hs, 2 * Ln), _arr(cref, cts, 2 * Ln), np.array(list(sw), dtype=np.uint8),
                             _arr(cref, ss, _words(s_bits)), s_bits, **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. K3
K3_SHAPES = [(128, 1, 1), (128, 2, 64), (128, 4, 128), (128, 8, 65), (264, 2, 88), (2048, 4, 130), (3072, 2, 64)]


@pytest.mark.parametrize("bits,K,s_bits", K3_SHAPES)
def test_k3_routes_records_and_outputs_equal_the_reference(eng, cref, bits, K, s_bits):
    n, hs, cts, ss = _inputs(bits, K, s_bits, 0x5d00 + bits + K)
    if K >= 4:
        assert set(_specials(s_bits)) < set(ss) and len(set(ss)) == K
    L = 2 * _words(bits)
    n2 = n * n
    perm = _perm(K, 0x5d01 + K)
    sw = XR.route(perm)                                           # the reference's bits: the device applies what it is given
    mixed, routes, steps = _smix(eng, cref, bits, n, hs, cts, sw, ss, s_bits)
    tr = XR.smix_trace(n, hs, cts, sw, ss, s_bits)
    assert tr.routed == [cts[p] for p in perm]
    assert tr.mixed == [cts[p] * pow(hs, s, n2) % n2 for p, s in zip(perm, ss)]
    assert [cref.limbs_to_int(row) for row in mixed] == tr.mixed
    per = XR.per_output(s_bits)
    assert routes.shape == (len(tr.layers), K, L) and steps.shape == (K, per, 4, L)
    for l, layer in enumerate(tr.layers):
        assert np.array_equal(routes[l], _arr(cref, layer, L)), "layer %d" % l
    want = np.stack([_arr(cref, st, L) for st in XR.records(tr)])
    bad = np.nonzero((steps.reshape(-1, 4, L) != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, "record %d differs" % bad[0]
    # where K is too small for them, 0, all ones and the lone top bit run in further calls on the same ciphertexts and bits
    rest = [v for v in dict.fromkeys(_specials(s_bits)) if v not in ss]
    assert (K >= 4) == (not rest)
    for at in range(0, len(rest), K):
        ss2 = (rest[at:at + K] + ss)[:K]
        mixed2, _, steps2 = _smix(eng, cref, bits, n, hs, cts, sw, ss2, s_bits, want_routes=False)
        tr2 = XR.smix_trace(n, hs, cts, sw, ss2, s_bits)
        assert [cref.limbs_to_int(row) for row in mixed2] == tr2.mixed == [cts[p] * pow(hs, s, n2) % n2 for p, s in zip(perm, ss2)]
        assert np.array_equal(steps2.reshape(-1, 4, L), np.stack([_arr(cref, st, L) for st in XR.records(tr2)])), ss2
    # the values only
    m2, none_r, none_s = _smix(eng, cref, bits, n, hs, cts, sw, ss, s_bits, want_steps=False, want_routes=False)
    assert none_r is None and none_s is None and np.array_equal(m2, mixed)
    # the product's own router gives the same outputs (its bits may differ from the reference's)
    m3, _, _ = _smix(eng, cref, bits, n, hs, cts, eng.mix_route(perm), ss, s_bits, want_steps=False)
    assert np.array_equal(m3, mixed)


def test_k3_values_through_fifteen_layers(eng, cref):
    bits, K, s_bits = 128, 256, 3
    n, hs, cts, ss = _inputs(bits, K, s_bits, 0x5d02)
    perm = _perm(K, 0x5d03)
    assert len(XR.benes_layers(K)) == 15 and set(ss) == set(range(8))
    mixed, routes, steps = _smix(eng, cref, bits, n, hs, cts, eng.mix_route(perm), ss, s_bits)
    assert routes.shape == (15, K, 4) and steps.shape == (K, 7, 4, 4)
    assert [cref.limbs_to_int(row) for row in routes[-1]] == [cts[p] for p in perm]
    assert [cref.limbs_to_int(row) for row in mixed] == [cts[p] * pow(hs, s, n * n) % (n * n) for p, s in zip(perm, ss)]
    assert [cref.limbs_to_int(row) for row in steps[:, 6, 0]] == [cts[p] for p in perm]          # every final block multiplies its d_i
    assert [cref.limbs_to_int(row) for row in steps[:, 6, 3]] == [cref.limbs_to_int(row) for row in mixed]


@pytest.mark.parametrize("bits,K,s_bits", [(128, 4, 70), (264, 2, 88)])
def test_k3_routes_and_chains_equal_the_existing_kernels_bit_for_bit(eng, cref, bits, K, s_bits):
    """the route layers are pz_paillier_mix's on the same cts and bits; an output's chain is chain 0 of pz_paillier_partial with v = hs,
    theta = s_i, e_bits = s_bits"""
    n, hs, cts, ss = _inputs(bits, K, s_bits, 0x5d04 + K)
    Ln = _words(bits)
    lim = cref.int_to_limbs
    sw = eng.mix_route(_perm(K, 0x5d05))
    mixed, routes, steps = _smix(eng, cref, bits, n, hs, cts, sw, ss, s_bits)
    _, mroutes, _ = eng.paillier_mix(Ln, lim(n, Ln), _arr(cref, cts, 2 * Ln), sw, _arr(cref, [1] * K, Ln), want_steps=False)
    assert routes.shape[0] == len(XR.benes_layers(K)) and np.array_equal(routes, mroutes)
    some_ct = np.stack([lim(hs, 2 * Ln)])
    for i in range(K):
        h, _, prec = eng.paillier_partial(Ln, lim(n, Ln), lim(hs, 2 * Ln), lim(ss[i], 2 * Ln), some_ct, s_bits)
        assert np.array_equal(prec[1:1 + 2 * s_bits], steps[i, :2 * s_bits])
        assert np.array_equal(steps[i, 2 * s_bits, 1], h.reshape(-1))                               # the final block's second operand
        assert cref.limbs_to_int(h) == pow(hs, ss[i], n * n)


def test_k3_refusals_in_order_with_untouched_outputs(eng, cref):
    from paillier_halo2_amd import _lib

    bits, K, s_bits = 128, 4, 70
    n, hs, cts, ss = _inputs(bits, K, s_bits, 0x5d06)
    lim = cref.int_to_limbs
    need = K * XR.per_output(s_bits)
    n_, h_, c_, s_ = lim(n, 2), lim(hs, 4), _arr(cref, cts, 4), _arr(cref, ss, 2)
    sw = np.array(XR.route(_perm(K, 0x5d07)), dtype=np.uint8)
    zero_n = lim(0, 2)
    routes = np.full((3, K, 4), 0xA5, dtype=np.uint64)
    steps = np.full((need, 4, 4), 0xA5, dtype=np.uint64)
    out = np.full((K, 4), 0xA5, dtype=np.uint64)

    def call(limbs=2, count=K, sb=s_bits, nn=n_, hh=h_, cc=c_, bb=sw, sv=s_, cap=need, oo=out, rr=routes):
        p = lambda a: None if a is None else a.ctypes.data
        return eng.L.pz_paillier_smix(eng.ctx, limbs, count, sb, p(nn), p(hh), p(cc), p(bb), p(sv), p(rr), p(steps), cap, p(oo))

    bad_bit = sw.copy()
    bad_bit[-1] = 2
    bad_s = s_.copy()
    bad_s[K - 1, 1] = 1 << 6                                                       # s_K = 2^70
    INV, UNS, CAP, MSG, ZERO, RNG = (_lib.PZ_ERR_INVALID, _lib.PZ_ERR_UNSUPPORTED, _lib.PZ_ERR_CAPACITY, _lib.PZ_ERR_MESSAGE_RANGE,
                                     _lib.PZ_ERR_ZERO_MODULUS, _lib.PZ_ERR_RANGE)
    # each refusal alone
    for kw in (dict(nn=None), dict(hh=None), dict(cc=None), dict(bb=None), dict(sv=None), dict(oo=None), dict(limbs=0), dict(count=0),
               dict(count=3), dict(count=6), dict(count=2048), dict(sb=0), dict(sb=257)):
        assert call(**kw) == INV, kw
    assert call(limbs=65) == UNS
    assert call(cap=need - 1) == CAP
    assert call(bb=bad_bit) == MSG
    assert call(sv=bad_s) == MSG
    assert call(nn=zero_n) == ZERO
    # the order: each one wins over all that follow it
    assert call(count=3, limbs=65, cap=0, bb=bad_bit, nn=zero_n) == INV
    assert call(sb=128 * 65 + 1, limbs=65, cap=0, bb=bad_bit, nn=zero_n) == INV
    assert call(limbs=65, cap=0, bb=bad_bit, nn=zero_n) == UNS
    assert call(cap=0, bb=bad_bit, nn=zero_n) == CAP
    assert call(bb=bad_bit, nn=zero_n) == MSG
    assert call(sv=bad_s, nn=zero_n) == MSG
    # an hs and a ciphertext of exactly n^2 are found by the kernel
    assert call(hh=lim(n * n, 4)) == RNG
    assert call(cc=_arr(cref, [cts[0], n * n, cts[2], cts[3]], 4)) == RNG
    assert (routes == 0xA5).all() and (steps == 0xA5).all() and (out == 0xA5).all()
    # the context serves an honest call afterwards; s_bits = 256 is the widest exponent of this key size
    assert call() == 0
    tr = XR.smix_trace(n, hs, cts, sw.tolist(), ss, s_bits)
    assert [cref.limbs_to_int(row) for row in out] == tr.mixed
    assert np.array_equal(routes, np.stack([_arr(cref, layer, 4) for layer in tr.layers]))
    assert tuple(cref.limbs_to_int(steps[-1, f]) for f in range(4)) == XR.records(tr)[-1]
    # K = 1 takes neither bits nor routes
    one = np.zeros((1, 4), dtype=np.uint64)
    assert call(count=1, bb=None, rr=None, oo=one) == 0 and cref.limbs_to_int(one[0]) == cts[0] * pow(hs, ss[0], n * n) % (n * n)
    # the Python layer reports the status
    assert _status(lambda: _smix(eng, cref, bits, n, hs, cts, bad_bit, ss, s_bits)) == MSG


@pytest.mark.parametrize("bits,K,s_bits", [(128, 1, 1), (128, 8, 65), (264, 2, 88)])
def test_k3_dev_form_equals_the_host_form(eng, cref, bits, K, s_bits):
    import torch
    from paillier_halo2_amd import _lib

    n, hs, cts, ss = _inputs(bits, K, s_bits, 0x5d08 + K)
    Ln = _words(bits)
    L = 2 * Ln
    lim = cref.int_to_limbs
    sw = eng.mix_route(_perm(K, 0x5d09))
    mixed, routes, steps = _smix(eng, cref, bits, n, hs, cts, sw, ss, s_bits)
    layers, per = routes.shape[0], steps.shape[1]
    d_routes = torch.zeros((max(layers, 1), K, L), dtype=torch.int64, device="cuda")
    d_steps = torch.zeros((K, per, 4, L), dtype=torch.int64, device="cuda")
    args = (Ln, lim(n, Ln), lim(hs, L), _arr(cref, cts, L), sw, _arr(cref, ss, _words(s_bits)), s_bits)
    got = eng.paillier_smix_dev(*args, d_routes.data_ptr(), d_steps.data_ptr(), K * per)
    assert np.array_equal(got, mixed)
    assert np.array_equal(d_routes.cpu().numpy().view(np.uint64)[:layers], routes)
    assert np.array_equal(d_steps.cpu().numpy().view(np.uint64), steps)
    assert np.array_equal(eng.paillier_smix_dev(*args, 0, 0, 0), mixed)                          # neither buffer: the values only
    assert _status(lambda: eng.paillier_smix_dev(*args, d_routes.data_ptr(), d_steps.data_ptr(), K * per - 1)) == _lib.PZ_ERR_CAPACITY


# ------------------------------------------------------------------------------------------------------------------ 2. end to end
def test_sballots_through_two_mixers_decrypt_in_the_predicted_order(eng, cref):
    """K = 4 sballots of distinct small values from pz_paillier_sballot go through two smix mixers with different permutations under
    the one key (n, hs); decryption of the second mixer's outputs gives the values in the order perm_2 o perm_1 predicts, with the
    randomness h^(s0 + s1 + s2), and no output is an input ciphertext"""
    from paillier_halo2_amd import keys

    bits, K, b, s_bits = 128, 4, 4, 100
    key = DR.key(bits)
    n, g = key[0], key[1]
    Ln = _words(bits)
    lim = cref.int_to_limbs
    rng = random.Random(0x5d0a)
    x = _unit(rng, n)
    hs = keys.djn_generator(eng, n, rand=lambda k_: x)
    assert hs == XR.djn_hs(n, x)
    h = XR.djn_h(n, x)
    ms = [5, 9, 2, 14]
    s0, s1, s2 = ([rng.randrange(1 << s_bits) for _ in range(K)] for _ in range(3))
    c0, _ = eng.paillier_sballot(Ln, lim(n, Ln), lim(g, Ln), lim(hs, 2 * Ln), np.array(ms, dtype=np.uint64), _arr(cref, s0, 2), b, s_bits,
                                 want_steps=False)
    cts0 = [cref.limbs_to_int(row) for row in c0]
    assert cts0 == [XR.encrypt(n, g, hs, m, s) for m, s in zip(ms, s0)]
    perm1, perm2 = [2, 0, 3, 1], [3, 2, 0, 1]
    mix = lambda c, perm, ss: eng.paillier_smix(Ln, lim(n, Ln), lim(hs, 2 * Ln), c, eng.mix_route(perm), _arr(cref, ss, 2), s_bits,
                                                want_steps=False, want_routes=False)[0]
    m1 = mix(c0, perm1, s1)
    m2 = mix(m1, perm2, s2)
    cts1, cts2 = ([cref.limbs_to_int(row) for row in m] for m in (m1, m2))
    assert not set(cts0) & set(cts1) and not set(cts0) & set(cts2) and not set(cts1) & set(cts2)
    sk = eng.paillier_sk(Ln, n, g, key[2], key[3])
    try:
        got, got_r, fl = eng.paillier_decrypt(sk, m2)
        assert fl.tolist() == [0] * K
        both = [perm1[perm2[i]] for i in range(K)]                    # output i of mixer 2 holds mixer 1's output perm2[i]
        assert [cref.limbs_to_int(row) for row in got] == [ms[j] for j in both] == [9, 14, 2, 5]
        assert [cref.limbs_to_int(row) for row in got_r] == [pow(h, s0[both[i]] + s1[perm2[i]] + s2[i], n) for i in range(K)]
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------------------------ 3. K4
SX4 = (128, 64, 13, 14, 4, 2)      # three layers, two limbs of s, break points crossed inside the chains
SX2 = (264, 88, 11, 14, 2, 1)      # the reference's add-test key size on 88-bit limbs: K3's fields are 10 words, K4's 9
SX1 = (128, 64, 10, 13, 1, 1)      # one ciphertext: no switch, a proven re-randomisation
SX2S = (128, 64, 10, 13, 2, 1)     # one switch


def _smix_inputs(bits, K, s_bits, seed):
    n = P.synth_paillier_inputs(bits, seed)[0]
    n, hs, cts, ss = _inputs(bits, K, s_bits, seed, n=n)
    return n, hs, cts, ss, _perm(K, seed + 3)


def _ref_trace(n, hs, cts, ss, sw, bits, W, sl, forge=None):
    return XR.smix_trace(n, hs, cts, sw, ss, sl * W, forge=forge, limb_bits=W, limbs=2 * (bits // W))


def _k3_dev(eng, cref, bits, n, hs, cts, sw, ss, s_bits):
    """pz_paillier_smix_dev's routes and records left on the device as they are -> (mixed integers, d_routes, d_steps)"""
    import torch

    wn = _words(bits)
    K = len(cts)
    per = XR.per_output(s_bits)
    layers = len(XR.benes_layers(K))
    d_routes = torch.zeros((max(layers, 1), K, 2 * wn), dtype=torch.int64, device="cuda")
    d_steps = torch.zeros((K, per, 4, 2 * wn), dtype=torch.int64, device="cuda")
    lim = cref.int_to_limbs
    mixed = eng.paillier_smix_dev(wn, lim(n, wn), lim(hs, 2 * wn), _arr(cref, cts, 2 * wn), np.array(list(sw), dtype=np.uint8),
                                  _arr(cref, ss, _words(s_bits)), s_bits, d_routes.data_ptr(), d_steps.data_ptr(), K * per)
    return [cref.limbs_to_int(row) for row in mixed], d_routes, d_steps


def _k4_inputs(cref, bits, s_bits, n, hs, cts, ss, res):
    lim = cref.int_to_limbs
    wn, wl = _words(bits), _words(2 * bits)
    return np.concatenate([lim(n, wn), lim(hs, wl)] + [lim(c, wl) for c in cts] + [lim(s, _words(s_bits)) for s in ss] + [lim(v, wl) for v in res])


@pytest.mark.parametrize("shape", [SX1, SX2S, SX4, SX2], ids=["K1", "K2", "K4", "264-88"])
def test_k4_dense_stream_and_break_point_columns_equal_the_reference(eng, cref, shape):
    import torch
    from paillier_halo2_amd import _lib, layout

    bits, W, lb, k, K, sl = shape
    s_bits = sl * W
    Ln, n_rows = bits // W, 1 << k
    n, hs, cts, ss, perm = _smix_inputs(bits, K, s_bits, 0x5d20 + K)
    sw = XR.route(perm)
    tr = _ref_trace(n, hs, cts, ss, sw, bits, W, sl)
    want_a, want_l, seg = XR.smix_cells(n, hs, cts, ss, tr.mixed, sl, bits, W, lb, tr)
    assert seg["satisfied"]
    na, nl = eng.smix_cells(Ln, W, lb, K, sl)
    assert (na, nl) == (len(want_a), len(want_l))
    cc = layout.circuit_cells("smix", Ln, W, lb, count=K, s_limbs=sl)
    assert (cc.advice, cc.lookup) == (na, nl)
    pub = eng.smix_public_cells(Ln, W, lb, K, sl).tolist()
    assert pub == XR.public_cells(K, sl, bits, W, lb) and len(pub) == Ln + 2 * Ln + 2 * K * 2 * Ln
    assert [want_a[c] for c in pub] == XR.statement(n, hs, cts, tr.mixed, bits, W)
    mixed, d_routes, d_steps = _k3_dev(eng, cref, bits, n, hs, cts, sw, ss, s_bits)
    assert mixed == tr.mixed
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    inputs = _k4_inputs(cref, bits, s_bits, n, hs, cts, ss, tr.mixed)
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.smix_expand_dev(Ln, W, lb, K, sl, inputs, sw, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d (network at %d, outputs at %d)" % (len(bad), bad[0], seg["network"][0], seg["outputs"][0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    # ---- the same stream in break-point columns
    rb = layout.row_budget(k)
    starts = layout.break_points(XR.smix_gate_mask(K, sl, bits, W, lb), rb.max_rows)
    A_used = starts.shape[0] - 1
    A, Lk = rb.columns_for(na, filled=A_used), rb.columns_for(nl)
    full = np.concatenate([starts, np.full(A - A_used, na, dtype=np.uint64)])
    d_starts = torch.from_numpy(full.astype(np.int64)).cuda()
    cols = torch.zeros((A + Lk + 1, n_rows, 4), dtype=torch.int64, device="cuda")
    eng.smix_expand_cols_dev(Ln, W, lb, K, sl, inputs, sw, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(),
                             cols[A].data_ptr(), d_starts.data_ptr(), A, rb.max_rows, rb.max_rows, n_rows)
    eng.sync()
    want_cols = XR.place(want_a, want_l, full, A, Lk, rb.max_rows, k, [])
    host = cols.cpu().numpy().view(np.uint64)
    for j in range(A + Lk + 1):
        assert cref.fr_mont_to_ints(host[j]) == want_cols[j], j
    assert A_used >= 2
    # a switch byte above 1 and an s_i of 2^s_bits are refused
    if K > 1:
        over = list(sw)
        over[0] = 2
        assert _status(lambda: eng.smix_expand_dev(Ln, W, lb, K, sl, inputs, over, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(),
                                                   d_adv.data_ptr(), d_lk.data_ptr())) == _lib.PZ_ERR_MESSAGE_RANGE
    if s_bits % 64:
        wide = _k4_inputs(cref, bits, s_bits, n, hs, cts, ss[:-1] + [1 << s_bits], tr.mixed)
        assert _status(lambda: eng.smix_expand_dev(Ln, W, lb, K, sl, wide, sw, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(),
                                                   d_adv.data_ptr(), d_lk.data_ptr())) == _lib.PZ_ERR_MESSAGE_RANGE
    # the by-kind entry points keep refusing kind 10; a count that is no power of two and an s of no or too many limbs have no stream
    assert _status(lambda: eng.circuit_cells(10, Ln, W, lb, 0, 2 * s_bits)) == _lib.PZ_ERR_INVALID
    assert _status(lambda: eng.smix_cells(Ln, W, lb, 3, sl)) == _lib.PZ_ERR_INVALID
    assert _status(lambda: eng.smix_cells(Ln, W, lb, K, 0)) == _lib.PZ_ERR_INVALID
    assert _status(lambda: eng.smix_cells(Ln, W, lb, K, 2 * Ln + 1)) == _lib.PZ_ERR_INVALID


def test_k4_dense_stream_of_a_mismatching_result_equals_the_reference(eng, cref):
    """output 1's claimed ciphertext differs from the computed one in a middle limb only, output 0's matches: the running-equality chain
    of output 1 drops there and stays down, the is_zero inverse cell of that limb is a true inverse"""
    import torch

    bits, W, lb, k, K, sl = SX2S
    s_bits = sl * W
    Ln = bits // W
    n, hs, cts, ss, perm = _smix_inputs(bits, K, s_bits, 0x5d2a)
    sw = XR.route(perm)
    tr = _ref_trace(n, hs, cts, ss, sw, bits, W, sl)
    res = [tr.mixed[0], tr.mixed[1] ^ (1 << (W + 5))]   # limb 1 of 4
    want_a, want_l, seg = XR.smix_cells(n, hs, cts, ss, res, sl, bits, W, lb, tr)
    assert not seg["satisfied"]
    na, nl = eng.smix_cells(Ln, W, lb, K, sl)
    assert (na, nl) == (len(want_a), len(want_l))
    mixed, d_routes, d_steps = _k3_dev(eng, cref, bits, n, hs, cts, sw, ss, s_bits)
    assert mixed == tr.mixed
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.smix_expand_dev(Ln, W, lb, K, sl, _k4_inputs(cref, bits, s_bits, n, hs, cts, ss, res), sw, d_routes.data_ptr(), d_steps.data_ptr(),
                        d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d (outputs at %d)" % (len(bad), bad[0], seg["outputs"][0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l


# ------------------------------------------------------------------------------------------------------------------ 4. structure
@pytest.mark.parametrize("shape", [SX4, SX2, SX1, SX2S], ids=["K4", "264-88", "K1", "K2"])
@pytest.mark.parametrize("expose", [False, True])
def test_native_structure_equals_the_python_generator(eng, shape, expose):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout, prover_native

    bits, W, lb, k, K, sl = shape
    sa = CS.stream_structure("smix", bits, W, lb, count=K, s_limbs=sl)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=expose)
    ns = prover_native.NativeStructure(eng, "smix", bits, W, lb, k, count=K, s_limbs=sl, expose=expose)
    try:
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], 0, 2 * sl * W)
        assert ns.starts().tolist() == starts.tolist()
        assert ns.starts()[: ns.n_adv_used + 1].tolist() == layout.break_points(XR.smix_gate_mask(K, sl, bits, W, lb), ns.max_rows).tolist()
        assert ns.constants() == [int(c) for c in cs.constants]
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        Ln = bits // W
        assert (ns.n_instance, ns.n_public) == ((1, Ln + 2 * Ln + 2 * K * 2 * Ln) if expose else (0, 0))
        if expose:
            assert ns.public_cells() == cs.public_cells
    finally:
        ns.free()
    for count, s_limbs in ((0, sl), (3, sl), (2048, sl), (K, 0), (K, 4 * (bits // W) + 1)):
        with pytest.raises(Exception):
            prover_native.NativeStructure(eng, "smix", bits, W, lb, k, count=count, s_limbs=s_limbs)


# ------------------------------------------------------------------------------------------------------------------ 5. / 6. the proof
class World:
    """SRS with a known toxic scalar, both structures with the instance column, both keys, witnesses from K3 -> K4; two elections'
    keys (n, hs) of one size"""

    def __init__(self, eng, cref, shape, seed):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.bits, self.W, self.lb, self.k, self.K, self.sl = shape
        bits, W, lb, k, K, sl = shape
        self.s_bits = sl * W
        self.n_rows = n = 1 << k
        self.a = _smix_inputs(bits, K, self.s_bits, seed)              # (n, hs, cts, ss, perm)
        self.b = _smix_inputs(bits, K, self.s_bits, seed + 16)         # another election's key, ciphertexts, exponents and permutation
        assert self.a[0] != self.b[0] and self.a[1] != self.b[1] and (K == 1 or self.a[4] != self.b[4])
        rng = random.Random(seed + 7)
        self.s_tox = rng.randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        self.ns = prover_native.NativeStructure(eng, "smix", bits, W, lb, k, count=K, s_limbs=sl, expose=True)
        self.sa = CS.stream_structure("smix", bits, W, lb, count=K, s_limbs=sl)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)
        self.structure = self.ns.download()

    def trace(self, el=None, forge=None, cts=None, sw=None):
        n, hs, cts_, ss, perm = self.a if el is None else el
        sw = XR.route(perm) if sw is None else sw
        return _ref_trace(n, hs, cts_ if cts is None else cts, ss, sw, self.bits, self.W, self.sl, forge=forge)

    def statement(self, trace, el=None, cts=None):
        n, hs, cts_, _, _ = self.a if el is None else el
        return XR.statement(n, hs, cts_ if cts is None else cts, trace.mixed, self.bits, self.W)

    def witness(self, el=None):
        """K4's columns [m'][2^k][4] from K3's routes and records, both left on the device"""
        import torch

        eng, cref, ns = self.eng, self.cref, self.ns
        n, hs, cts, ss, perm = self.a if el is None else el
        sw = eng.mix_route(perm)                                        # the product's own router
        mixed, d_routes, d_steps = _k3_dev(eng, cref, self.bits, n, hs, cts, sw, ss, self.s_bits)
        d_mod = torch.from_numpy(cref.int_to_limbs(n ** 2, _words(2 * self.bits)).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        eng.smix_expand_cols_dev(self.bits // self.W, self.W, self.lb, self.K, self.sl, _k4_inputs(cref, self.bits, self.s_bits, n, hs, cts, ss, mixed),
                                 sw, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(),
                                 ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, self.n_rows)
        eng.sync()
        return cols

    def reference_columns(self, trace, el=None, cts=None):
        n, hs, cts_, ss, _ = self.a if el is None else el
        want_a, want_l, _ = XR.smix_cells(n, hs, cts_ if cts is None else cts, ss, trace.mixed, self.sl, self.bits, self.W, self.lb, trace)
        return XR.place(want_a, want_l, self.ns.starts(), self.ns.n_adv, self.ns.n_lk, self.ns.max_rows, self.k, [])

    def upload(self, ref):
        """reference columns (integers) as a device witness [m][2^k][4]: the advice and lookup columns; the rest is the prover's"""
        import torch

        cols = torch.zeros((self.ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        for j in range(self.ns.n_adv + self.ns.n_lk):
            cols[j] = torch.from_numpy(self.cref.fr_ints_to_mont(ref[j]).astype(np.int64)).cuda()
        return cols

    def ints(self, cols):
        host = cols.cpu().numpy().view(np.uint64)
        return [self.cref.fr_mont_to_ints(host[j]) for j in range(self.ns.m)]

    def check(self, ints, instances):
        """tally_ref.check_columns and oracle.circuit.mock_prover on a witness under the NATIVE structure"""
        ns = self.ns
        sel, mc, mr = self.structure
        ck = ns.n_adv + ns.n_lk
        ints = list(ints)
        ints[ck] = [c % R for c in ns.constants()] + ints[ck][ns.n_constants:]
        ints[ck + 1] = list(instances) + ints[ck + 1][len(instances):]
        bad = XR.check_columns(sel, mc, mr, range(1 << self.lb), ints, ns.n_lk)
        # the MockProver analogue of oracle/circuit.py finds fault with the same witnesses, for the same reasons
        mock = XR.mock_prover(sel, mc, mr, ints, ns.n_lk, self.k, self.lb)
        assert {m.split()[0] for m in mock} == {t for t, _, _ in bad}
        return bad

    def close(self):
        self.key.free()
        self.ns.free()
        self.bl.free()
        self.bm.free()


@pytest.fixture(scope="module")
def world(eng, cref):
    w = World(eng, cref, SX4, 0x5d30)
    yield w
    w.close()


def _oracle_checks(cref, w, pr, seed, inst):
    """oracle/verifier.py's checks with the statement in the transcript: the identity at x from the evaluations, SHPLONK's final identity"""
    from oracle import verifier as V
    from paillier_halo2_amd import prover

    A, Lk, m = w.ns.n_adv, w.ns.n_lk, w.ns.m
    S = -(-m // 2)
    ev = {f: PR.ints_of(cref, v) for f, v in pr.evals.items()}
    ch = PR.replay_challenges_pub(seed, inst, pr.commitments, pr.evals)
    inst_x = PR.instance_eval(w.k, inst, ch["x"])
    ident = PR.expected_h_pub(w.k, BF, A, Lk, prover.CHUNK, ev, ch["beta"], ch["gamma"], ch["y"], ch["x"], prover.DELTA, inst_x) == ev["h"][0][0]
    xn = pow(ch["x"], w.n_rows, R)
    hc = cref.g1_normalize(cref.msm_g1(cref.fr_ints_to_mont([pow(xn, i, R) for i in range(3)]), pr.commitments["h"]))
    vk_c = w.key.vk_commitments()
    com = dict(pr.commitments)
    com.update(fixed=vk_c["fixed"], sigma=vk_c["sigma"], h=[hc])
    opening = V.shplonk_check(cref, PR.query_layout_pub(A, Lk, m, S), prover.rotation_points(w.pk.dom, ch["x"]), com, ev, ch["sh_y"], ch["sh_v"],
                              ch["sh_u"], pr.commitments["w1"][0], pr.commitments["w2"][0], w.s_tox)
    return pr.h_degree_ok, ident, opening


def test_device_witness_satisfies_the_native_structure(eng, cref, world):
    w = world
    cols = w.witness()
    tr = w.trace()
    inst = w.ns.gather_public(cols.data_ptr())
    assert inst == w.statement(tr) and len(inst) == 2 + 4 + 2 * 4 * 4
    ints = w.ints(cols)
    ref = w.reference_columns(w.trace(sw=eng.mix_route(w.a[4]).tolist()))        # (the witness was routed by the product)
    for j in range(w.ns.n_adv + w.ns.n_lk):
        assert ints[j] == ref[j], j
    assert w.check(ints, inst) == []
    assert w.ns.n_adv_used >= 40                            # break points are crossed inside every chain
    # the two keys describe one circuit
    a, b = w.key.vk_commitments(), w.pk.vk_commitments()
    assert np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])


def test_connected_proof_both_provers_two_elections_one_key(eng, cref, world):
    """two mixes with different n, hs, permutations and s are proven by both provers under ONE proving key and verified under ONE
    verifying key: the property kind 8 cannot have, whose r^n chains carry n's bits in the key's shape"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    tr_a, tr_b = w.trace(), w.trace(w.b)
    good, other = w.statement(tr_a), w.statement(tr_b, w.b)
    kw = dict(enc_bits=w.bits, limb_bits=w.W)
    assert PV.public_inputs("smix", n=w.a[0], hs=w.a[1], cts=w.a[2], mixed=tr_a.mixed, **kw) == good
    assert PV.public_inputs("smix", n=w.b[0], hs=w.b[1], cts=w.b[2], mixed=tr_b.mixed, **kw) == other != good
    seeds = [b"smix-stepper-a", b"smix-python-a", b"smix-stepper-b", b"smix-python-b"]
    cols_a, cols_b = w.witness(), w.witness(w.b)
    assert w.ns.gather_public(cols_b.data_ptr()) == other
    assert w.check(w.ints(cols_b), other) == []
    p0 = prover_native.create_proof(w.key, cols_a.data_ptr(), prover.HashTranscript(seeds[0]), seed=5, instances=good)
    p1 = prover.create_proof(w.pk, w.witness(), prover.HashTranscript(seeds[1]), seed=6, tile=8, instances=good)
    p2 = prover_native.create_proof(w.key, cols_b.data_ptr(), prover.HashTranscript(seeds[2]), seed=7, instances=other)      # the SAME key
    p3 = prover.create_proof(w.pk, w.witness(w.b), prover.HashTranscript(seeds[3]), seed=8, tile=8, instances=other)
    proofs, inst = [p0, p1, p2, p3], [good, good, other, other]
    for pr, seed, st in zip(proofs, seeds, inst):
        assert _oracle_checks(cref, w, pr, seed, st) == (True, True, True)
    assert PV.verify_batch(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True] * 4)
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True] * 4)
    # election A's proofs under election B's statement
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[other] * 4) == (False, [False, False, True, True])
    # ... and against `mixed` with two entries exchanged: the proof names which output stands where
    swapped = PV.public_inputs("smix", n=w.a[0], hs=w.a[1], cts=w.a[2], mixed=[tr_a.mixed[1], tr_a.mixed[0]] + tr_a.mixed[2:], **kw)
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[swapped, swapped, other, other]) == (False, [False, False, True, True])


def test_one_proven_rerandomisation(eng, cref):
    """K = 1: c' holds what c holds"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = World(eng, cref, SX1, 0x5d40)
    try:
        n, hs, cts, ss, _ = w.a
        tr = w.trace()
        assert tr.mixed == [cts[0] * pow(hs, ss[0], n * n) % (n * n)] and tr.layers == []
        cols = w.witness()
        inst = PV.public_inputs("smix", n=n, hs=hs, cts=cts, mixed=tr.mixed, enc_bits=w.bits, limb_bits=w.W)
        assert w.ns.gather_public(cols.data_ptr()) == inst == w.statement(tr)
        assert w.check(w.ints(cols), inst) == []
        seed = b"smix-one"
        pr = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=3, instances=inst)
        assert PV.verify_batch(eng, w.params, w.vk, [pr], [seed], instances=[inst]) == (True, [True])
        other = PV.public_inputs("smix", n=n, hs=hs, cts=cts, mixed=[tr.mixed[0] ^ 1], enc_bits=w.bits, limb_bits=w.W)
        assert PV.verify_batch(eng, w.params, w.vk, [pr], [seed], instances=[other]) == (False, [False])
    finally:
        w.close()


FORGES = [("bit", 1, 0, 2), ("dup", 0, 1), ("src", 1, 2, 1), ("in", 3, 1), ("s", 0, 5), ("base", 3, 1), ("hss", 2, 1), ("d", 1, 1)]
FORGE_IDS = ["switch-bit-is-2", "selects-under-different-bits", "select-reads-limb+1", "layer-0-reads-c+1", "chain-run-with-another-s",
             "chain-first-sq-is-hs+1", "final-operand-is-hss+1", "final-operand-is-d+1"]


@pytest.mark.parametrize("forge", FORGES, ids=FORGE_IDS)
def test_forged_edges_are_rejected(eng, cref, world, forge):
    """a switch bit of 2; a switch whose selects run under different bits (one input twice, one dropped); a select reading the previous
    layer's limb + 1; layer 0 reading c_4 + 1 under the exposed c_4; chain 0 run consistently with s' = 5 while assign_integer(s_0)
    keeps s_0; chain 3's first sq taken as hs + 1; the final block fed hss + 1, or d + 1 -- each with everything downstream, the claimed
    outputs and the statement recomputed consistently, placed in the NATIVE structure's columns.  Every lookup and every final equality
    holds; a copy constraint objects (the bit of 2: assert_bit's gate).  For the dup and the s a proof made from the forged witness is
    refused by verification."""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    n, hs, cts, ss, perm = w.a
    sw = None
    if forge[0] == "bit":       # equal inputs at the forged switch: the bit of 2 changes no value, assert_bit's gate ALONE objects
        cts, sw = [cts[0], cts[1], cts[0], cts[3]], [0] * 6
    ft = w.trace(forge=forge, cts=cts, sw=sw)
    honest = w.trace(cts=cts, sw=sw)
    assert (ft.mixed != honest.mixed) == (forge[0] != "bit")
    inst = w.statement(ft, cts=cts)
    assert inst == PV.public_inputs("smix", n=n, hs=hs, cts=cts, mixed=ft.mixed, enc_bits=w.bits, limb_bits=w.W)    # a statement a verifier accepts
    ref = w.reference_columns(ft, cts=cts)
    bad = w.check(ref + [[0] * w.n_rows], inst)
    assert bad and {t for t, _, _ in bad} == ({"gate"} if forge[0] == "bit" else {"copy"})
    if forge[0] in ("dup", "s"):
        seed = b"smix-forged"
        cols = w.upload(ref)
        assert w.ns.gather_public(cols.data_ptr()) == inst
        hcols = w.upload(w.reference_columns(honest, cts=cts))
        hinst = w.statement(honest, cts=cts)
        pf = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=inst)
        ph = prover_native.create_proof(w.key, hcols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=hinst)
        assert not pf.h_degree_ok and ph.h_degree_ok
        assert PV.verify_batch(eng, w.params, w.vk, [pf, ph], [seed, seed], instances=[inst, hinst]) == (False, [False, True])
