"""GPU: T-of-T threshold decryption (circuit kind 7 / "partial") through every layer -- a trustee's chains
under its secret share (K3), the combiner, the cell stream (K4), the native structure generator, and connected proofs "h = v^theta and
u = (c^2)^theta for one theta" by both provers -- against the independent restatement of tests/partial_ref.py in Python integers.
Every comparison is exact.

Main shape SP1: 128-bit n from two 64-bit safe primes, 64-bit limbs, lookup_bits 13 (the ballot's), K = 1: two chains of 256 bits, 1025
mul_mod blocks, 1.24 million cells.  k = 14 is the smallest k that fits: the lookup table needs lookup_bits < k, so k = 13 is refused
(asserted in World); at k = 14 the stream takes 76 advice and 9 lookup columns."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import partial_ref as TR

pytestmark = pytest.mark.gpu

R = P.FR_R


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


def _inputs(bits, K, seed):
    """n of `bits` bits, v and K ciphertexts below n^2 (K3 asks no more of them): 1, n^2 - 1 where K allows, random otherwise"""
    rng = random.Random(seed)
    n = P.synth_paillier_inputs(bits, seed)[0]
    n2 = n * n
    v = rng.randrange(2, n2)
    special = [n2 - 1, 1]
    cts = [special[i - 1] if 1 <= i < 3 else rng.randrange(2, n2) for i in range(K)]
    return n, v, cts


def _thetas(e_bits, seed, full):
    """a share with its top bit set; where `full`, zero and all ones too"""
    rng = random.Random(seed)
    top = (1 << (e_bits - 1)) | rng.getrandbits(e_bits - 1) if e_bits > 1 else 1
    return [top, 0, (1 << e_bits) - 1] if full else [top]


def _k3(eng, cref, bits, n, v, theta, cts, e_bits, want_steps=True):
    Ln = _words(bits)
    lim = cref.int_to_limbs
    return eng.paillier_partial(Ln, lim(n, Ln), lim(v, 2 * Ln), lim(theta, 2 * Ln), np.stack([lim(c, 2 * Ln) for c in cts]), e_bits,
                                want_steps=want_steps)


def _record_array(cref, recs, L):
    return np.stack([np.stack([cref.int_to_limbs(x, L) for x in st]) for st in recs])


# ------------------------------------------------------------------------------------------------------------------ 1. K3
# one bit; the exponent's word boundary (64, 65); the circuit's own length; a partial last word; the real size (E = 1); E = 2
K3_SHAPES = [(128, 1, 1), (128, 1, 64), (128, 2, 65), (128, 3, 256), (264, 1, 100), (2048, 1, 4096), (3072, 1, 130)]


@pytest.mark.parametrize("bits,K,e_bits", K3_SHAPES)
def test_k3_records_h_and_u_equal_the_reference(eng, cref, bits, K, e_bits):
    n, v, cts = _inputs(bits, K, 0x7a10 + 64 * K + e_bits)
    L = 2 * _words(bits)
    n2 = n * n
    for theta in _thetas(e_bits, bits + e_bits, full=bits == 128 and e_bits <= 65):
        h, u, steps = _k3(eng, cref, bits, n, v, theta, cts, e_bits)
        tr = TR.partial_trace(n, v, theta, cts, e_bits)
        want = TR.records(tr)
        assert steps.shape == (TR.n_records(K, e_bits), 4, L) and len(want) == steps.shape[0]
        assert cref.limbs_to_int(h) == tr.h == pow(v, theta, n2)
        assert [cref.limbs_to_int(row) for row in u] == tr.us == [pow(c * c % n2, theta, n2) for c in cts]
        bad = np.nonzero((steps != _record_array(cref, want, L)).any(axis=(1, 2)))[0]
        assert bad.size == 0, "record %d differs" % bad[0]
        h2, u2, none = _k3(eng, cref, bits, n, v, theta, cts, e_bits, want_steps=False)
        assert none is None and np.array_equal(h2, h) and np.array_equal(u2, u)


@pytest.mark.parametrize("e_bits", [1, 64])
def test_k3_chain_equals_the_weighted_tally_chain(eng, cref, e_bits):
    """for e_bits <= 64 chain j's records are pz_paillier_wtally's chain on the base c_j^2 with the weight theta"""
    bits, K = 128, 2
    n, v, cts = _inputs(bits, K, 0x7a20 + e_bits)
    Ln = _words(bits)
    lim = cref.int_to_limbs
    n2 = n * n
    theta = _thetas(e_bits, 0x7a21, False)[0]
    _, u, steps = _k3(eng, cref, bits, n, v, theta, cts, e_bits)
    bases = [v] + [c * c % n2 for c in cts]
    power, wsteps = eng.paillier_wtally(Ln, lim(n, Ln), np.stack([lim(b, 2 * Ln) for b in bases]),
                                        np.array([theta] * (K + 1), dtype=np.uint64), e_bits)
    wsteps = wsteps.reshape(-1, 4, 2 * Ln)
    assert np.array_equal(steps[K:], wsteps[: (K + 1) * 2 * e_bits])


def test_k3_refusals(eng, cref):
    from paillier_halo2_amd import _lib

    bits, K, e_bits = 128, 2, 65
    n, v, cts = _inputs(bits, K, 0x7a22)
    theta = _thetas(e_bits, 0x7a23, False)[0]
    lim = cref.int_to_limbs
    n_, v_, t_, c_ = lim(n, 2), lim(v, 4), lim(theta, 4), np.stack([lim(c, 4) for c in cts])
    need = TR.n_records(K, e_bits)
    steps = np.zeros((need, 4, 4), dtype=np.uint64)
    h = np.zeros(4, dtype=np.uint64)
    u = np.zeros((K, 4), dtype=np.uint64)

    def call(limbs=2, count=K, eb=e_bits, cap=need, n=n_, v=v_, t=t_, c=c_, st=steps, h=h, u=u):
        p = lambda a: None if a is None else a.ctypes.data
        return eng.L.pz_paillier_partial(eng.ctx, limbs, count, eb, p(n), p(v), p(t), p(c), p(st), cap, p(h), p(u))

    for kw in (dict(n=None), dict(v=None), dict(t=None), dict(c=None), dict(h=None), dict(u=None), dict(limbs=0), dict(count=0),
               dict(count=1025), dict(eb=0), dict(eb=257)):
        assert call(**kw) == _lib.PZ_ERR_INVALID, kw
    assert call(limbs=65) == _lib.PZ_ERR_UNSUPPORTED                       # 2 * limbs_n > 128 (refused before anything is read)
    assert call(cap=need - 1) == _lib.PZ_ERR_CAPACITY
    assert call(t=lim(1 << e_bits, 4)) == _lib.PZ_ERR_MESSAGE_RANGE        # theta = 2^e_bits
    assert call(t=lim(1 << 255, 4)) == _lib.PZ_ERR_MESSAGE_RANGE
    assert call(n=lim(0, 2)) == _lib.PZ_ERR_ZERO_MODULUS
    assert call(cap=need - 1, t=lim(1 << e_bits, 4), n=lim(0, 2)) == _lib.PZ_ERR_CAPACITY          # the order of the refusals
    assert call(t=lim(1 << e_bits, 4), n=lim(0, 2)) == _lib.PZ_ERR_MESSAGE_RANGE
    assert not steps.any() and not h.any() and not u.any()                 # refused before any launch: nothing was written
    # a base or a ciphertext >= n^2 travels through the kernel
    assert call(v=lim(n * n, 4)) == _lib.PZ_ERR_RANGE
    assert call(c=np.stack([lim(cts[0], 4), lim(n * n + 1, 4)])) == _lib.PZ_ERR_RANGE
    # the context serves an honest call afterwards
    steps[:] = 0
    assert call() == 0
    tr = TR.partial_trace(n, v, theta, cts, e_bits)
    assert cref.limbs_to_int(h) == tr.h and [cref.limbs_to_int(row) for row in u] == tr.us
    assert np.array_equal(steps, _record_array(cref, TR.records(tr), 4))
    assert _status(lambda: eng.paillier_partial(2, n_, v_, lim(1 << e_bits, 4), c_, e_bits)) == _lib.PZ_ERR_MESSAGE_RANGE


# ------------------------------------------------------------------------------------------------------------------ 2. the combiner
def _deal(p, q, T, seed, g=None):
    """the reference's dealing: (n, g, lam, shares, mu2)"""
    import math

    rng = random.Random(seed)
    n = p * q
    lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    g = n + 1 if g is None else g
    theta = TR.theta_of(p, q)
    return n, g, lam, TR.split(theta, n * lam, T, rng.randrange), TR.mu2_of(n, g, theta)


def _encrypt(n, g, ms, rng):
    return [P.paillier_enc_native(n, g, m, rng.randrange(1, n)) for m in ms]


@pytest.mark.parametrize("T", [1, 2, 3, 7])
@pytest.mark.parametrize("K", [1, 4])
def test_combiner_equals_the_reference_and_the_full_key(eng, cref, T, K):
    from tests import decrypt_ref as DR

    bits = 128
    p, q = DR.primes(bits)
    rng = random.Random(0x7a30 + 16 * T + K)
    g = None if K == 1 else DR.key(bits, standard_g=False, seed=3)[1]      # a general g: a != 1 in mu2
    n, g, lam, shares, mu2 = _deal(p, q, T, 0x7a31 + T, g)
    Ln = _words(bits)
    lim = cref.int_to_limbs
    ms = [0, 1, n - 1, rng.randrange(n)][:K] if K > 1 else [rng.randrange(n)]
    cts = _encrypt(n, g, ms, rng)
    parts = [[TR.partial(c, s, n) for c in cts] for s in shares]
    arr = np.stack([np.stack([lim(u, 2 * Ln) for u in row]) for row in parts])
    m, flags = eng.paillier_combine(Ln, lim(n, Ln), lim(mu2, Ln), arr)
    want = [TR.combine([parts[i][j] for i in range(T)], n, mu2) for j in range(K)]
    assert flags.tolist() == [0] * K and [cref.limbs_to_int(row) for row in m] == [w[0] for w in want] == ms
    sk = eng.paillier_sk(Ln, n, g, lam, pow(n, -1, lam))
    try:
        m_full, _, fl = eng.paillier_decrypt(sk, np.stack([lim(c, 2 * Ln) for c in cts]), want_r=False)
        assert fl.tolist() == [0] * K and np.array_equal(m_full, m)
    finally:
        sk.free()


def test_combiner_flags(eng, cref):
    """a partial replaced by another trustee's sets flag bit 0 for exactly the entries it touches; a partial >= n^2 is PZ_ERR_RANGE with
    the other entries still written; the device form agrees"""
    import torch
    from paillier_halo2_amd import _lib
    from tests import decrypt_ref as DR

    bits, T, K = 128, 3, 4
    p, q = DR.primes(bits)
    rng = random.Random(0x7a40)
    n, g, lam, shares, mu2 = _deal(p, q, T, 0x7a41)
    Ln = _words(bits)
    lim = cref.int_to_limbs
    ms = [5, 0, n - 1, rng.randrange(n)]
    cts = _encrypt(n, g, ms, rng)
    parts = [[TR.partial(c, s, n) for c in cts] for s in shares]
    to_arr = lambda pp: np.stack([np.stack([lim(u, 2 * Ln) for u in row]) for row in pp])
    swapped = [list(row) for row in parts]
    swapped[1][2] = parts[0][2]                                            # trustee 1's partial of entry 2 := trustee 0's
    m, flags = eng.paillier_combine(Ln, lim(n, Ln), lim(mu2, Ln), to_arr(swapped))
    assert TR.combine([swapped[i][2] for i in range(T)], n, mu2) == (0, 1)
    assert flags.tolist() == [0, 0, 1, 0] and [cref.limbs_to_int(row) for row in m] == [ms[0], ms[1], 0, ms[3]]
    over = [list(row) for row in parts]
    over[2][1] = n * n
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        eng.paillier_combine(Ln, lim(n, Ln), lim(mu2, Ln), to_arr(over))
    assert e.value.status == _lib.PZ_ERR_RANGE
    assert e.value.flags.tolist() == [0, 2, 0, 0] and [cref.limbs_to_int(row) for row in e.value.m] == [ms[0], 0, ms[2], ms[3]]
    # the device form: asynchronous on the context's stream, the flags are the caller's to read
    d_parts = torch.from_numpy(to_arr(over).astype(np.int64)).cuda()
    d_m = torch.zeros((K, Ln), dtype=torch.int64, device="cuda")
    d_fl = torch.zeros(K, dtype=torch.uint8, device="cuda")
    eng.paillier_combine_dev(Ln, lim(n, Ln), lim(mu2, Ln), K, T, d_parts.data_ptr(), d_m.data_ptr(), d_fl.data_ptr())
    eng.sync()
    assert d_fl.cpu().tolist() == [0, 2, 0, 0] and np.array_equal(d_m.cpu().numpy().view(np.uint64), e.value.m)
    # refusals before any launch
    for count, trustees in ((0, T), (1025, T), (K, 0), (K, 257)):
        assert eng.L.pz_paillier_combine(eng.ctx, Ln, count, trustees, lim(n, Ln).ctypes.data, lim(mu2, Ln).ctypes.data,
                                         to_arr(parts).ctypes.data, m.ctypes.data, flags.ctypes.data) == _lib.PZ_ERR_INVALID
    assert _status(lambda: eng.paillier_combine(Ln, lim(0, Ln), lim(mu2, Ln), to_arr(parts))) == _lib.PZ_ERR_ZERO_MODULUS


def test_ballots_tally_partials_combine_to_the_vote_counts(eng, cref):
    """end to end, value level: two voters' ballots over K = 2 candidates (pz_paillier_ballot), one pz_paillier_tally per candidate,
    three trustees' pz_paillier_partial under a key from keys.deal_shares, pz_paillier_combine: the vote counts"""
    from paillier_halo2_amd import keys

    bits, T = 128, 3
    rng = random.Random(0x7a50)
    key, shares = keys.deal_shares(TR.SAFE_P, TR.SAFE_Q, T, rand=rng.randrange)
    assert key.v_order_proved and key.n.bit_length() == bits
    n, Ln = key.n, _words(bits)
    lim = cref.int_to_limbs
    votes = [[1, 0], [1, 0]]                                               # both voters choose candidate 0
    ballots = []
    for ms in votes:
        rs = np.stack([lim(rng.randrange(1, n), Ln) for _ in ms])
        c, _, _ = eng.paillier_ballot(Ln, lim(n, Ln), lim(key.g, Ln), np.array(ms, dtype=np.uint64), rs, 1, want_steps=False)
        ballots.append(c)
    totals = np.stack([eng.paillier_tally(Ln, lim(n, Ln), np.stack([b[j] for b in ballots]), want_steps=False)[0] for j in range(2)])
    e_bits = 2 * bits                                                      # the circuit's own length, 2 enc_bits
    parts = []
    for i, s in enumerate(shares):
        h, u, _ = eng.paillier_partial(Ln, lim(n, Ln), lim(key.v, 2 * Ln), lim(s, 2 * Ln), totals, e_bits, want_steps=False)
        assert cref.limbs_to_int(h) == key.hs[i]
        parts.append(u)
    m, flags = eng.paillier_combine(Ln, lim(n, Ln), lim(key.mu2, Ln), np.stack(parts))
    assert flags.tolist() == [0, 0] and [cref.limbs_to_int(row) for row in m] == [2, 0]


# ------------------------------------------------------------------------------------------------------------------ 3. K4
SP1 = (128, 64, 13, 14, 1)
SP2 = (264, 88, 11, 14, 1)          # the reference's add-test key size on 88-bit limbs: K3 writes 10 words a field, K4 reads 9
SP3 = (128, 64, 10, 13, 2)          # two ciphertexts: a squaring block between two chains twice


def _circuit_inputs(bits, K, seed):
    """as _inputs, with a share of the circuit's 2 enc_bits bits whose top bit is set"""
    n, v, cts = _inputs(bits, K, seed)
    rng = random.Random(seed + 1)
    theta = (1 << (2 * bits - 1)) | (rng.getrandbits(2 * bits - 1) & ~1)
    return n, v, theta, cts


def _device_records(eng, cref, bits, n, v, theta, cts, trace=None):
    """the K + (K + 1) 4 bits records on the device, fields of ceil(2 bits / 64) words: K3's own (trace = None) or a given trace's"""
    import torch

    L64 = _words(2 * bits)
    if trace is None:
        Ln = _words(bits)
        lim = cref.int_to_limbs
        n_rec = TR.n_records(len(cts), 2 * bits)
        d = torch.zeros((n_rec, 4, 2 * Ln), dtype=torch.int64, device="cuda")
        h, u = eng.paillier_partial_dev(Ln, lim(n, Ln), lim(v, 2 * Ln), lim(theta, 2 * Ln), np.stack([lim(c, 2 * Ln) for c in cts]), 2 * bits,
                                        d.data_ptr(), n_rec)
        tr = TR.partial_trace(n, v, theta, cts, 2 * bits)
        assert cref.limbs_to_int(h) == tr.h and [cref.limbs_to_int(row) for row in u] == tr.us
        if 2 * Ln == L64:
            return d                                         # the records as pz_paillier_partial_dev left them
        assert not bool(d[:, :, L64:].any())
        return d[:, :, :L64].contiguous()
    rec = np.stack([np.stack([cref.int_to_limbs(x, L64) for x in st]) for st in TR.records(trace)])
    return torch.from_numpy(rec.astype(np.int64)).cuda()


def _partial_inputs(cref, bits, n, v, theta, cts, h, us):
    lim = cref.int_to_limbs
    wn, wl = _words(bits), _words(2 * bits)
    return np.concatenate([lim(n, wn), lim(v, wl), lim(theta, wl)] + [lim(c, wl) for c in cts] + [lim(h, wl)] + [lim(u, wl) for u in us])


@pytest.mark.parametrize("shape", [SP1, SP2, SP3], ids=["SP1", "264-88", "K2"])
def test_k4_dense_stream_and_break_point_columns_equal_the_reference(eng, cref, shape):
    import torch
    from paillier_halo2_amd import _lib, layout

    bits, W, lb, k, K = shape
    Ln, n_rows = bits // W, 1 << k
    n, v, theta, cts = _circuit_inputs(bits, K, 0x7a60 + K)
    tr = TR.partial_trace(n, v, theta, cts, 2 * bits)
    want_a, want_l, seg = TR.partial_cells(n, v, theta, cts, tr.h, tr.us, bits, W, lb, tr)
    assert seg["satisfied"]
    na, nl = eng.partial_cells(Ln, W, lb, K)
    assert (na, nl) == (len(want_a), len(want_l))
    pub = eng.partial_public_cells(Ln, W, lb, K).tolist()
    assert len(pub) == Ln + (2 + 2 * K) * 2 * Ln
    assert [want_a[c] for c in pub] == TR.statement(n, v, tr.h, cts, tr.us, bits, W)
    d_steps = _device_records(eng, cref, bits, n, v, theta, cts)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    inputs = _partial_inputs(cref, bits, n, v, theta, cts, tr.h, tr.us)
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.partial_expand_dev(Ln, W, lb, K, inputs, d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    # a share that does not fit the circuit's 2 enc_bits bits is refused (264-bit n: its 9 words hold 576 bits, 528 count)
    if 2 * bits % 64:
        over = _partial_inputs(cref, bits, n, v, 1 << (2 * bits), cts, tr.h, tr.us)
        assert _status(lambda: eng.partial_expand_dev(Ln, W, lb, K, over, d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(),
                                                      d_lk.data_ptr())) == _lib.PZ_ERR_MESSAGE_RANGE
    for count in (0, 1025):
        assert _status(lambda: eng.partial_cells(Ln, W, lb, count)) == _lib.PZ_ERR_INVALID
    # the by-kind entry points keep refusing kind 7
    assert _status(lambda: eng.circuit_cells(7, Ln, W, lb, 4 * bits, 0)) == _lib.PZ_ERR_INVALID
    if shape is SP2:
        return      # (4 million cells: the column cut does not depend on the limb width, the two other shapes hold it)
    # ---- the same stream in break-point columns
    rb = layout.row_budget(k)
    starts = layout.break_points(TR.partial_gate_mask(K, bits, W, lb), rb.max_rows)
    A_used = starts.shape[0] - 1
    A, Lk = rb.columns_for(na, filled=A_used), rb.columns_for(nl)
    full = np.concatenate([starts, np.full(A - A_used, na, dtype=np.uint64)])
    d_starts = torch.from_numpy(full.astype(np.int64)).cuda()
    cols = torch.zeros((A + Lk + 1, n_rows, 4), dtype=torch.int64, device="cuda")
    eng.partial_expand_cols_dev(Ln, W, lb, K, inputs, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(), cols[A].data_ptr(),
                                d_starts.data_ptr(), A, rb.max_rows, rb.max_rows, n_rows)
    eng.sync()
    want_cols = TR.place(want_a, want_l, full, A, Lk, rb.max_rows, k, [])
    host = cols.cpu().numpy().view(np.uint64)
    for j in range(A + Lk + 1):
        assert cref.fr_mont_to_ints(host[j]) == want_cols[j], j
    assert A_used >= 2


def test_k4_dense_stream_of_a_mismatching_result_equals_the_reference(eng, cref):
    """result 1 (u_1) as claimed differs from chain 1's in a middle limb only, h and u_2 match: the running-equality chain of result 1
    drops there and stays down, the is_zero inverse cell of that limb is a true inverse -- the cells the matching streams above never
    reach"""
    import torch

    bits, W, lb, k, K = SP3
    Ln = bits // W
    n, v, theta, cts = _circuit_inputs(bits, K, 0x7a6a)
    tr = TR.partial_trace(n, v, theta, cts, 2 * bits)
    us = [tr.us[0] ^ (1 << (W + 5)), tr.us[1]]          # limb 1 of 4
    want_a, want_l, seg = TR.partial_cells(n, v, theta, cts, tr.h, us, bits, W, lb, tr)
    assert not seg["satisfied"]
    na, nl = eng.partial_cells(Ln, W, lb, K)
    assert (na, nl) == (len(want_a), len(want_l))
    d_steps = _device_records(eng, cref, bits, n, v, theta, cts)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.partial_expand_dev(Ln, W, lb, K, _partial_inputs(cref, bits, n, v, theta, cts, tr.h, us), d_steps.data_ptr(), d_mod.data_ptr(),
                           d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d (results at %d)" % (len(bad), bad[0], seg["results"][0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l


# ------------------------------------------------------------------------------------------------------------------ 4. structure
@pytest.mark.parametrize("shape", [SP1, SP3], ids=["SP1", "K2"])
@pytest.mark.parametrize("expose", [False, True])
def test_native_structure_equals_the_python_generator(eng, shape, expose):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout, prover_native

    bits, W, lb, k, K = shape
    sa = CS.stream_structure("partial", bits, W, lb, count=K)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=expose)
    ns = prover_native.NativeStructure(eng, "partial", bits, W, lb, k, count=K, expose=expose)
    try:
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], 4 * bits, 0)
        assert ns.starts().tolist() == starts.tolist()
        assert ns.starts()[: ns.n_adv_used + 1].tolist() == layout.break_points(TR.partial_gate_mask(K, bits, W, lb), ns.max_rows).tolist()
        assert ns.constants() == [int(c) for c in cs.constants]
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        Ln = bits // W
        assert (ns.n_instance, ns.n_public) == ((1, Ln + (2 + 2 * K) * 2 * Ln) if expose else (0, 0))
        if expose:
            assert ns.public_cells() == cs.public_cells
    finally:
        ns.free()
    for count in (0, 1025):
        with pytest.raises(Exception):
            prover_native.NativeStructure(eng, "partial", bits, W, lb, k, count=count)


# ------------------------------------------------------------------------------------------------------------------ 5. the proofs
T = 3


class World:
    """SP1: a threshold key for T = 3 trustees dealt by keys.deal_shares over two hard-coded 64-bit safe primes, one ciphertext, SRS with a
    known toxic scalar, both structures with the instance column, both keys (ONE each for all trustees), witnesses from K3 -> K4"""

    def __init__(self, eng, cref):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import keys, prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.bits, self.W, self.lb, self.k, self.K = SP1
        bits, W, lb, k, K = SP1
        self.n_rows = n = 1 << k
        rng = random.Random(0x7a70)
        self.tkey, self.shares = keys.deal_shares(TR.SAFE_P, TR.SAFE_Q, T, rand=rng.randrange)
        assert self.tkey.v_order_proved and self.tkey.n.bit_length() == bits
        self.nn, self.v = self.tkey.n, self.tkey.v
        self.msg = 0x1234567
        self.cts = [P.paillier_enc_native(self.nn, self.tkey.g, self.msg, rng.randrange(1, self.nn))]
        self.s_tox = rng.randrange(2, R)
        F = lambda x: cref.fr_ints_to_mont([x % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        with pytest.raises(Exception):                       # lookup_bits < k: k = 13 does not fit, k = 14 is the smallest
            prover_native.NativeStructure(eng, "partial", bits, W, lb, k - 1, count=K, expose=True)
        self.ns = prover_native.NativeStructure(eng, "partial", bits, W, lb, k, count=K, expose=True)
        self.sa = CS.stream_structure("partial", bits, W, lb, count=K)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)
        self.structure = self.ns.download()

    def trace(self, i, forge=None):
        return TR.partial_trace(self.nn, self.v, self.shares[i], self.cts, 2 * self.bits, forge=forge)

    def statement(self, trace, h=None):
        return TR.statement(self.nn, self.v, trace.h if h is None else h, self.cts, trace.us, self.bits, self.W)

    def witness(self, i):
        """trustee i's columns [m][2^k][4]: K3's records on the device, expanded by K4 into the native structure's break-point columns"""
        import torch

        eng, cref, ns = self.eng, self.cref, self.ns
        tr = self.trace(i)
        d_steps = _device_records(eng, cref, self.bits, self.nn, self.v, self.shares[i], self.cts)
        d_mod = torch.from_numpy(cref.int_to_limbs(self.nn ** 2, _words(2 * self.bits)).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        eng.partial_expand_cols_dev(self.bits // self.W, self.W, self.lb, self.K,
                                    _partial_inputs(cref, self.bits, self.nn, self.v, self.shares[i], self.cts, tr.h, tr.us), d_steps.data_ptr(),
                                    d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows,
                                    self.n_rows)
        eng.sync()
        return cols

    def reference_columns(self, i, trace, inst):
        want_a, want_l, _ = TR.partial_cells(self.nn, self.v, self.shares[i], self.cts, trace.h, trace.us, self.bits, self.W, self.lb, trace)
        return TR.place(want_a, want_l, self.ns.starts(), self.ns.n_adv, self.ns.n_lk, self.ns.max_rows, self.k, [], inst)

    def ints(self, cols):
        host = cols.cpu().numpy().view(np.uint64)
        return [self.cref.fr_mont_to_ints(host[j]) for j in range(self.ns.m)]

    def check(self, ints, instances):
        """tally_ref.check_columns on a witness under the NATIVE structure"""
        ns = self.ns
        sel, mc, mr = self.structure
        ck = ns.n_adv + ns.n_lk
        ints = list(ints)
        ints[ck] = [c % R for c in ns.constants()] + ints[ck][ns.n_constants:]
        ints[ck + 1] = list(instances) + ints[ck + 1][len(instances):]
        return TR.check_columns(sel, mc, mr, range(1 << self.lb), ints, ns.n_lk)

    def close(self):
        self.key.free()
        self.ns.free()
        self.bl.free()
        self.bm.free()


@pytest.fixture(scope="module")
def world(eng, cref):
    w = World(eng, cref)
    yield w
    w.close()


def test_device_witness_satisfies_the_native_structure(eng, cref, world):
    w = world
    cols = w.witness(0)
    tr = w.trace(0)
    assert tr.h == w.tkey.hs[0]
    inst = w.ns.gather_public(cols.data_ptr())
    assert inst == w.statement(tr) and len(inst) == 2 + 4 * 4
    ints = w.ints(cols)
    ref = w.reference_columns(0, tr, inst)
    for j in range(w.ns.n_adv + w.ns.n_lk):
        assert ints[j] == ref[j], j
    assert w.check(ints, inst) == []
    assert w.ns.n_adv_used >= 70                            # break points are crossed inside every chain
    # the two keys describe one circuit
    a, b = w.key.vk_commitments(), w.pk.vk_commitments()
    assert np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])


def test_connected_proofs_three_trustees_both_provers_one_key(eng, cref, world):
    """each of the T = 3 trustees proves its partial decryption of the one ciphertext through both provers under ONE key; the six proofs
    verify in one batch call with their instances; the combiner opens the partials to the message; a proof checked against another
    trustee's h is refused"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    kw = dict(enc_bits=w.bits, limb_bits=w.W)
    proofs, seeds, insts, partials = [], [], [], []
    for i in range(T):
        tr = w.trace(i)
        inst = w.statement(tr)
        assert PV.public_inputs("partial", n=w.nn, v=w.v, h=w.tkey.hs[i], cts=w.cts, partials=tr.us, **kw) == inst
        cols = w.witness(i)
        assert w.ns.gather_public(cols.data_ptr()) == inst
        s0, s1 = b"partial-stepper-%d" % i, b"partial-python-%d" % i
        proofs.append(prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(s0), seed=5 + i, instances=inst))
        proofs.append(prover.create_proof(w.pk, w.witness(i), prover.HashTranscript(s1), seed=15 + i, tile=8, instances=inst))
        seeds += [s0, s1]
        insts += [inst, inst]
        partials.append(tr.us)
    assert all(p.h_degree_ok for p in proofs)
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=insts) == (True, [True] * (2 * T))          # pz_verify_batch_pub
    wire = [PV.proof_to_bytes(eng, w.vk, p) for p in proofs]
    assert PV.verify_batch_bytes(eng, w.params, w.vk, wire, seeds, instances=insts) == (True, [True] * (2 * T))
    # trustee 0's proofs against trustee 1's h (everything else its own); trustee 2's against a partial changed by one
    wrong = list(insts)
    wrong[0] = wrong[1] = w.statement(w.trace(0), h=w.tkey.hs[1])
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=wrong) == (False, [False, False] + [True] * 4)
    plus = list(insts)
    plus[4] = plus[5] = plus[4][:-8] + TR.statement(w.nn, w.v, w.tkey.hs[2], w.cts, [partials[2][0] ^ 1], w.bits, w.W)[-8:]
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=plus) == (False, [True] * 4 + [False, False])
    # the verified partials combine to the message
    Ln = _words(w.bits)
    lim = cref.int_to_limbs
    m, flags = eng.paillier_combine(Ln, lim(w.nn, Ln), lim(w.tkey.mu2, Ln), np.stack([np.stack([lim(u, 2 * Ln) for u in us]) for us in partials]))
    assert flags.tolist() == [0] and cref.limbs_to_int(m[0]) == w.msg


FORGES = [("exp", 1, None), ("base", 1), ("ct", 1, 1), ("sq", 1, 1), ("res", 0, 1)]


@pytest.mark.parametrize("forge", FORGES, ids=["chain-run-with-theta+1", "first-sq-is-v+1", "square-of-c+1", "first-sq-is-s+1", "result-is-h+1"])
def test_forged_edges_are_rejected(eng, cref, world, forge):
    """one forge per copy constraint of the circuit: chain 1 run with theta + 1 while assign_integer(theta) keeps theta; chain 0's first sq
    taken as v + 1; the squaring block fed c + 1; chain 1's first sq taken as s + 1; the assert_equal_fresh of chain 0 fed its result + 1
    -- each with everything downstream, the claimed h and u and the statement recomputed consistently, so every gate, every lookup and
    every final equality holds.  A copy constraint of the NATIVE structure objects, and nothing else does"""
    w = world
    theta = w.shares[0]
    if forge[0] == "exp":
        forge = ("exp", 1, theta + 1 if theta + 1 < 1 << (2 * w.bits) else theta - 1)
    ft, honest = w.trace(0, forge=forge), w.trace(0)
    assert (ft.h, ft.us) != (honest.h, honest.us)
    inst = w.statement(ft)
    bad = w.check(w.reference_columns(0, ft, inst), inst)
    assert bad and {t for t, _, _ in bad} == {"copy"}
