"""GPU: the packed ballot (kind 11 / "pballot") through every layer -- the entries' K slot chains, hs-chain
and folds (K3), the slot bases read from one trace, the cell stream (K4), the native structure generator, and connected proofs with
the statement "these R ciphertexts are (prod_j G_j^v_ij) hs^s_i under (n, hs) and the bases G_j = g^(2^(j w)), every v_ij below 2^b,
every s_i below 2^s_bits, and the values of ciphertext i add up to S_i" by both provers, two elections with DIFFERENT n, g, hs and slot
width proven with ONE proving key -- against the independent restatement of tests/pballot_ref.py in Python integers.  Every comparison
is exact.

Main shape PB1: 128-bit n, 64-bit limbs, lookup_bits 13, k = 14, R = 2, K = 3, b = 2, w = 8, s_limbs = 2 -- 542 blocks, an odd K with
two sum gates per ciphertext, an s that crosses a limb, break points crossed inside the chains."""
import math
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import pballot_ref as BR
from tests import public_ref as PR

pytestmark = pytest.mark.gpu

R = P.FR_R
BF = 6
#      bits  W  lb   k  R  K  b   w  sl
PB1 = (128, 64, 13, 14, 2, 3, 2, 8, 2)
PB2 = (264, 88, 11, 14, 1, 2, 1, 16, 1)     # the reference's add-test key size on 88-bit limbs: K3's fields are repacked
PB3 = (128, 64, 10, 13, 1, 1, 1, 8, 1)      # one ciphertext of one slot: no sum, no S


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _unit(rng, n):
    while True:
        x = rng.randrange(2, n)
        if math.gcd(x, n) == 1:
            return x


def _specials(bits_):
    return [0, (1 << bits_) - 1, 1 << (bits_ - 1)]           # zero, all ones, a lone top bit


def _inputs(bits, Rn, K, b, w, s_bits, seed):
    """-> (n, g, hs, gs, vs, ss).  values: 0, 2^b - 1, a lone top bit, then random below 2^b, ciphertext-major; s: the same three of
    s_bits bits in another order, then random"""
    rng = random.Random(seed)
    n, g = P.synth_paillier_inputs(bits, seed)[:2]
    hs = BR.djn_hs(n, _unit(rng, n))
    flat = [_specials(b)[i] if i < 3 else rng.randrange(1 << b) for i in range(Rn * K)]
    vs = [flat[i * K:(i + 1) * K] for i in range(Rn)]
    ss = [_specials(s_bits)[(i + 1) % 3] if i < 3 else rng.randrange(1 << s_bits) for i in range(Rn)]
    return n, g, hs, BR.bases(n, g, K, w), vs, ss


def _words(bits):
    return -(-bits // 64)


def _u64(ws):
    return np.array([int(w) for w in ws], dtype=np.uint64)


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


def _k3(eng, cref, bits, n, hs, gs, vs, ss, b, s_bits, want_steps=True):
    Ln = _words(bits)
    lim = cref.int_to_limbs
    return eng.paillier_pballot(Ln, lim(n, Ln), lim(hs, 2 * Ln), np.stack([lim(gj, 2 * Ln) for gj in gs]), np.stack([_u64(row) for row in vs]),
                                np.stack([lim(s, _words(s_bits)) for s in ss]), b, s_bits, want_steps=want_steps)


# ------------------------------------------------------------------------------------------------------------------ 1. K3
K3_SHAPES = [(128, 1, 1, 1, 1), (128, 1, 64, 1, 64), (128, 2, 3, 2, 128), (128, 100, 10, 1, 65), (264, 2, 5, 3, 88), (2048, 2, 3, 2, 130),
             (3072, 1, 2, 1, 64)]


@pytest.mark.parametrize("bits,Rn,K,b,s_bits", K3_SHAPES)
def test_k3_records_equal_the_reference(eng, cref, bits, Rn, K, b, s_bits):
    w = max(b, min(8, (bits - 1) // K))
    assert K * w < bits
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, K, b, w, s_bits, 0xb120 + 64 * K + b + s_bits)
    vectors = [(vs, ss)]
    if Rn * K == 1:     # one entry carries one value and one s: zero, all ones, the lone top bit and a random one each get a run
        rng = random.Random(bits + b + s_bits)
        sv_, sx = _specials(b), _specials(s_bits)
        vectors = [([[sv_[0]]], [sx[0]]), ([[sv_[1]]], [sx[1]]), ([[sv_[2]]], [sx[2]]), ([[rng.randrange(1 << b)]], [rng.randrange(1 << s_bits)])]
    L = 2 * _words(bits)
    per = BR.per_entry(K, b, s_bits)
    assert per == 2 * b * K + 2 * s_bits + K
    for vv, sv in vectors:
        c, steps = _k3(eng, cref, bits, n, hs, gs, vv, sv, b, s_bits)
        tr = BR.pballot_trace(n, hs, gs, vv, sv, b, s_bits)
        want = BR.records(tr)
        assert steps.shape == (Rn, per, 4, L) and len(want) == Rn * per
        assert [cref.limbs_to_int(row) for row in c] == tr.cts == [BR.encrypt(n, g, hs, row, w, s) for row, s in zip(vv, sv)]
        flat = steps.reshape(-1, 4, L)
        want_arr = np.stack([np.stack([cref.int_to_limbs(v, L) for v in st]) for st in want])
        bad = np.nonzero((flat != want_arr).any(axis=(1, 2)))[0]
        assert bad.size == 0, "record %d differs" % bad[0]
        c2, none = _k3(eng, cref, bits, n, hs, gs, vv, sv, b, s_bits, want_steps=False)
        assert none is None and np.array_equal(c2, c)


def test_k3_equals_the_parents_kernels_bit_for_bit(eng, cref):
    """with K = 1 and G_0 = g the records are pz_paillier_sballot's; slot j's chain is chain 0 of pz_paillier_partial on v = G_j with
    theta = v_ij over e_bits = b"""
    bits, Rn, b, s_bits = 128, 3, 2, 70
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, 1, b, 8, s_bits, 0xb121)
    Ln = _words(bits)
    lim = cref.int_to_limbs
    assert gs == [g]
    c, steps = _k3(eng, cref, bits, n, hs, gs, vs, ss, b, s_bits)
    c_s, steps_s = eng.paillier_sballot(Ln, lim(n, Ln), lim(g, Ln), lim(hs, 2 * Ln), _u64([row[0] for row in vs]),
                                        np.stack([lim(s, _words(s_bits)) for s in ss]), b, s_bits)
    assert np.array_equal(c, c_s) and np.array_equal(steps, steps_s)
    Rn, K = 2, 3
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, K, b, 8, s_bits, 0xb122)
    c, steps = _k3(eng, cref, bits, n, hs, gs, vs, ss, b, s_bits)
    some_ct = np.stack([lim(hs, 2 * Ln)])
    for i in range(Rn):
        for j in range(K):
            h, _, prec = eng.paillier_partial(Ln, lim(n, Ln), lim(gs[j], 2 * Ln), lim(vs[i][j], 2 * Ln), some_ct, b)
            assert np.array_equal(prec[1:1 + 2 * b], steps[i, 2 * b * j:2 * b * (j + 1)]), (i, j)
            assert cref.limbs_to_int(h) == pow(gs[j], vs[i][j], n * n)


@pytest.mark.parametrize("bits,K,w", [(128, 5, 12), (128, 3, 40), (128, 1, 100), (128, 2, 63), (264, 3, 64), (264, 2, 16), (2048, 4, 100)])
def test_bases_from_one_trace_equal_python_integers(eng, bits, K, w):
    from paillier_halo2_amd import keys

    n, g = P.synth_paillier_inputs(bits, 0xb130 + K)[:2]
    assert (1 << (K * w)) <= n
    got = keys.pballot_bases(eng, n, g, K, w)
    assert got == [pow(g, 1 << (j * w), n * n) for j in range(K)] == BR.bases(n, g, K, w)
    with pytest.raises(ValueError):
        keys.pballot_bases(eng, n, g, K + 1, (bits // (K + 1)) + 1)      # 2^(K w) > n


def test_k3_refusals_in_their_order(eng, cref):
    from paillier_halo2_amd import _lib

    bits, Rn, K, b, s_bits = 128, 2, 3, 2, 65
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, K, b, 8, s_bits, 0xb123)
    lim = cref.int_to_limbs
    sw = _words(s_bits)
    n_, h_, g_, v_, s_ = lim(n, 2), lim(hs, 4), np.stack([lim(gj, 4) for gj in gs]), np.stack([_u64(r) for r in vs]), np.stack([lim(s, sw) for s in ss])
    zero_n = lim(0, 2)
    v_bad = v_.copy()
    v_bad[1, 2] = 1 << b                                          # the LAST value is exactly 2^b
    s_bad = np.stack([lim(s, sw) for s in [ss[0], 1 << s_bits]])  # an s of exactly 2^s_bits: bit 1 of its second word
    per = BR.per_entry(K, b, s_bits)
    need = Rn * per
    steps = np.zeros((need, 4, 4), dtype=np.uint64)
    out = np.zeros((Rn, 4), dtype=np.uint64)

    def call(limbs=2, count=Rn, slots=K, mb=b, sb=s_bits, nn=n_, hh=h_, gg=g_, vv=v_, sv=s_, cap=need, st=steps, o=out):
        ptr = lambda a: None if a is None else a.ctypes.data
        return eng.L.pz_paillier_pballot(eng.ctx, limbs, count, slots, mb, sb, ptr(nn), ptr(hh), ptr(gg), ptr(vv), ptr(sv), ptr(st), cap, ptr(o))

    # 1. PZ_ERR_INVALID, ahead of everything else (here together with what the later checks would refuse)
    for kw in (dict(nn=None), dict(gg=None), dict(hh=None), dict(vv=None), dict(sv=None), dict(o=None), dict(limbs=0), dict(count=0),
               dict(count=1025), dict(slots=0), dict(slots=65), dict(count=342, slots=3), dict(count=17, slots=64), dict(mb=0), dict(mb=65),
               dict(sb=0), dict(sb=128 * 2 + 1)):
        assert call(**kw) == _lib.PZ_ERR_INVALID, kw
    assert call(limbs=65, count=0, cap=0) == _lib.PZ_ERR_INVALID
    # 2. PZ_ERR_UNSUPPORTED ahead of the capacity (2 * limbs_n > 128: refused before anything is read)
    assert call(limbs=65, cap=0) == _lib.PZ_ERR_UNSUPPORTED
    # 3. PZ_ERR_CAPACITY ahead of the ranges
    assert call(cap=need - 1, vv=v_bad, sv=s_bad, nn=zero_n) == _lib.PZ_ERR_CAPACITY
    # 4. PZ_ERR_MESSAGE_RANGE ahead of the zero modulus: a value, then an s
    assert call(vv=v_bad, nn=zero_n) == _lib.PZ_ERR_MESSAGE_RANGE
    assert call(sv=s_bad, nn=zero_n) == _lib.PZ_ERR_MESSAGE_RANGE
    # 5. PZ_ERR_ZERO_MODULUS
    assert call(nn=zero_n) == _lib.PZ_ERR_ZERO_MODULUS
    assert not steps.any() and not out.any()
    # hs >= n^2 or ANY G_j >= n^2: PZ_ERR_RANGE from the kernel's range bit, in both forms; nothing is written
    g_last = g_.copy()
    g_last[K - 1] = lim(n * n, 4)
    g_first = g_.copy()
    g_first[0] = lim(n * n + 1, 4)
    assert call(hh=lim(n * n, 4)) == _lib.PZ_ERR_RANGE
    assert call(gg=g_last) == _lib.PZ_ERR_RANGE
    assert call(gg=g_first) == _lib.PZ_ERR_RANGE
    assert call(gg=g_last, st=None, cap=0) == _lib.PZ_ERR_RANGE
    assert not steps.any() and not out.any()
    import torch

    d_steps = torch.zeros((need, 4, 4), dtype=torch.int64, device="cuda")
    assert _status(lambda: eng.paillier_pballot_dev(2, n_, lim(n * n + 5, 4), g_, v_, s_, b, s_bits, d_steps.data_ptr(), need)) == _lib.PZ_ERR_RANGE
    assert _status(lambda: eng.paillier_pballot_dev(2, n_, h_, g_last, v_, s_, b, s_bits, d_steps.data_ptr(), need)) == _lib.PZ_ERR_RANGE
    assert not bool(d_steps.any())
    # the Engine's wrapper raises the same statuses
    assert _status(lambda: eng.paillier_pballot(2, n_, h_, g_, v_bad, s_, b, s_bits)) == _lib.PZ_ERR_MESSAGE_RANGE
    assert _status(lambda: eng.paillier_pballot(2, n_, h_, g_, v_, s_bad, b, s_bits)) == _lib.PZ_ERR_MESSAGE_RANGE
    # ... and the context serves an honest call afterwards, in both forms
    assert call() == 0
    tr = BR.pballot_trace(n, hs, gs, vs, ss, b, s_bits)
    assert [cref.limbs_to_int(row) for row in out] == tr.cts
    assert tuple(cref.limbs_to_int(steps[-1, f]) for f in range(4)) == BR.records(tr)[-1]
    c = eng.paillier_pballot_dev(2, n_, h_, g_, v_, s_, b, s_bits, d_steps.data_ptr(), need)
    assert [cref.limbs_to_int(row) for row in c] == tr.cts
    assert np.array_equal(d_steps.cpu().numpy().view(np.uint64), steps)


# ------------------------------------------------------------------------------------------------------------------ 2. K4
def _device_records(eng, cref, bits, n, hs, gs, vs, ss, b, s_bits, trace=None):
    """the R (2 b K + 2 s_bits + K) records on the device AS K3 LEAVES THEM, fields of 2 ceil(bits / 64) words: K3's own (trace = None),
    or a given trace's (the forged ones)"""
    import torch

    rw = 2 * _words(bits)
    lim = cref.int_to_limbs
    if trace is None:
        c, rec = _k3(eng, cref, bits, n, hs, gs, vs, ss, b, s_bits)
        assert [cref.limbs_to_int(row) for row in c] == BR.pballot_trace(n, hs, gs, vs, ss, b, s_bits).cts
        rec = rec.reshape(-1, 4, rw)
    else:
        rec = np.stack([np.stack([lim(v, rw) for v in st]) for st in BR.records(trace)])
    return torch.from_numpy(np.ascontiguousarray(rec).astype(np.int64)).cuda()


def _pballot_inputs(cref, bits, s_bits, n, hs, gs, vs, ss, res):
    lim = cref.int_to_limbs
    wn, wl = _words(bits), _words(2 * bits)
    return np.concatenate([lim(n, wn), lim(hs, wl)] + [lim(gj, wl) for gj in gs] + [_u64([v for row in vs for v in row])] +
                          [lim(s, _words(s_bits)) for s in ss] + [lim(v, wl) for v in res])


@pytest.mark.parametrize("shape", [PB1, PB2, PB3], ids=["PB1", "264-88", "R1K1"])
def test_k4_dense_stream_and_break_point_columns_equal_the_reference(eng, cref, shape):
    import torch
    from paillier_halo2_amd import _lib, layout

    bits, W, lb, k, Rn, K, b, w, sl = shape
    s_bits = sl * W
    Ln, n_rows = bits // W, 1 << k
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, K, b, w, s_bits, 0xb124)
    tr = BR.pballot_trace(n, hs, gs, vs, ss, b, s_bits)
    want_a, want_l, seg = BR.pballot_cells(n, hs, gs, vs, ss, tr.cts, b, sl, bits, W, lb)
    assert seg["satisfied"] and ("sums" in seg) == (K >= 2)
    na, nl = eng.pballot_cells(Ln, W, lb, Rn, K, b, sl)
    assert (na, nl) == (len(want_a), len(want_l))
    pub = eng.pballot_public_cells(Ln, W, lb, Rn, K, b, sl).tolist()
    assert len(pub) == Ln + 2 * Ln * (1 + K + Rn) + (K >= 2) * Rn
    assert [want_a[c] for c in pub] == BR.statement(n, hs, gs, tr.cts, [sum(r) for r in vs] if K >= 2 else None, bits, W)
    d_steps = _device_records(eng, cref, bits, n, hs, gs, vs, ss, b, s_bits)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    inputs = _pballot_inputs(cref, bits, s_bits, n, hs, gs, vs, ss, tr.cts)
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.pballot_expand_dev(Ln, W, lb, Rn, K, b, sl, inputs, d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    # ---- the same stream in break-point columns
    rb = layout.row_budget(k)
    starts = layout.break_points(BR.pballot_gate_mask(Rn, K, b, sl, bits, W, lb), rb.max_rows)
    A_used = starts.shape[0] - 1
    A, Lk = rb.columns_for(na, filled=A_used), rb.columns_for(nl)
    full = np.concatenate([starts, np.full(A - A_used, na, dtype=np.uint64)])
    d_starts = torch.from_numpy(full.astype(np.int64)).cuda()
    cols = torch.zeros((A + Lk + 1, n_rows, 4), dtype=torch.int64, device="cuda")
    eng.pballot_expand_cols_dev(Ln, W, lb, Rn, K, b, sl, inputs, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(), cols[A].data_ptr(),
                                d_starts.data_ptr(), A, rb.max_rows, rb.max_rows, n_rows)
    eng.sync()
    want_cols = BR.place(want_a, want_l, full, A, Lk, rb.max_rows, k, [])
    host = cols.cpu().numpy().view(np.uint64)
    for j in range(A + Lk + 1):
        assert cref.fr_mont_to_ints(host[j]) == want_cols[j], j
    assert A_used >= 2
    # a value that does not fit m_bits and an s that does not fit s_bits are refused by both forms (s_bits = 88: bit 24 of word 1)
    last = [row[:] for row in vs]
    last[-1][-1] = 1 << b
    over = [_pballot_inputs(cref, bits, s_bits, n, hs, gs, last, ss, tr.cts)]
    if s_bits % 64:
        bad_s = _pballot_inputs(cref, bits, s_bits, n, hs, gs, vs, ss, tr.cts)
        bad_s[_words(bits) + (1 + K) * _words(2 * bits) + Rn * K + _words(s_bits) - 1] |= np.uint64(1 << (s_bits % 64))
        over.append(bad_s)
    for inp in over:
        assert _status(lambda: eng.pballot_expand_dev(Ln, W, lb, Rn, K, b, sl, inp, d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(),
                                                      d_lk.data_ptr())) == _lib.PZ_ERR_MESSAGE_RANGE
        assert _status(lambda: eng.pballot_expand_cols_dev(Ln, W, lb, Rn, K, b, sl, inp, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(),
                                                           cols[A].data_ptr(), d_starts.data_ptr(), A, rb.max_rows, rb.max_rows,
                                                           n_rows)) == _lib.PZ_ERR_MESSAGE_RANGE
    # the by-kind entry points refuse kind 11
    assert _status(lambda: eng.circuit_cells(11, Ln, W, lb, 2 * b, 2 * s_bits)) == _lib.PZ_ERR_INVALID


def test_k4_dense_stream_of_a_mismatching_result_equals_the_reference(eng, cref):
    """ciphertext 1's claimed value differs from the computed one in a middle limb only, ciphertext 0's matches: the running-equality
    chain of entry 1 drops there and stays down, the is_zero inverse cell of that limb is a true inverse -- the cells the matching
    streams above never reach"""
    import torch

    bits, W, lb, Rn, K, b, w, sl = 128, 64, 10, 2, 2, 2, 8, 1
    s_bits = sl * W
    Ln = bits // W
    n, g, hs, gs, vs, ss = _inputs(bits, Rn, K, b, w, s_bits, 0xb12a)
    tr = BR.pballot_trace(n, hs, gs, vs, ss, b, s_bits)
    res = [tr.cts[0], tr.cts[1] ^ (1 << (W + 5))]       # limb 1 of 4
    want_a, want_l, seg = BR.pballot_cells(n, hs, gs, vs, ss, res, b, sl, bits, W, lb)
    assert not seg["satisfied"]
    na, nl = eng.pballot_cells(Ln, W, lb, Rn, K, b, sl)
    assert (na, nl) == (len(want_a), len(want_l))
    d_steps = _device_records(eng, cref, bits, n, hs, gs, vs, ss, b, s_bits)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.pballot_expand_dev(Ln, W, lb, Rn, K, b, sl, _pballot_inputs(cref, bits, s_bits, n, hs, gs, vs, ss, res), d_steps.data_ptr(),
                           d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l


# ------------------------------------------------------------------------------------------------------------------ 3. structure
@pytest.mark.parametrize("shape", [PB1, PB3], ids=["PB1", "R1K1"])
@pytest.mark.parametrize("expose", [False, True])
def test_native_structure_equals_the_python_generator(eng, shape, expose):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout, prover_native

    bits, W, lb, k, Rn, K, b, w, sl = shape
    sa = CS.stream_structure("pballot", bits, W, lb, count=Rn, slots=K, m_bits=b, s_limbs=sl)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=expose)
    ns = prover_native.NativeStructure(eng, "pballot", bits, W, lb, k, count=Rn, slots=K, m_bits=b, s_limbs=sl, expose=expose)
    try:
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], 2 * b, 2 * sl * W)
        assert ns.starts().tolist() == starts.tolist()
        assert ns.starts()[: ns.n_adv_used + 1].tolist() == layout.break_points(BR.pballot_gate_mask(Rn, K, b, sl, bits, W, lb), ns.max_rows).tolist()
        assert ns.constants() == [int(c) for c in cs.constants]
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        Ln = bits // W
        assert (ns.n_instance, ns.n_public) == ((1, Ln + 2 * Ln * (1 + K + Rn) + (K >= 2) * Rn) if expose else (0, 0))
        if expose:
            assert ns.public_cells() == cs.public_cells
    finally:
        ns.free()
    for count, slots, m_bits, s_limbs in ((0, K, b, sl), (1025, 1, b, sl), (Rn, 0, b, sl), (Rn, 65, b, sl), (513, 2, b, sl), (Rn, K, 0, sl),
                                          (Rn, K, 65, sl), (Rn, K, b, 0), (Rn, K, b, 2 * (bits // W) + 1)):
        with pytest.raises(Exception):
            prover_native.NativeStructure(eng, "pballot", bits, W, lb, k, count=count, slots=slots, m_bits=m_bits, s_limbs=s_limbs)


# ------------------------------------------------------------------------------------------------------------------ 4. / 5. the proof
class World:
    """PB1: SRS with a known toxic scalar, both structures with the instance column, both keys -- made from the SHAPE alone, no key and
    no slot width of an election enters --, witnesses from K3 -> K4"""

    def __init__(self, eng, cref):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.bits, self.W, self.lb, self.k, self.R, self.K, self.b, self.w, self.sl = PB1
        bits, W, lb, k, Rn, K, b, w, sl = PB1
        self.s_bits = sl * W
        self.n_rows = n = 1 << k
        nn, g, hs, gs, _, ss = _inputs(bits, Rn, K, b, w, self.s_bits, 0xb130)
        self.elec_a = (nn, g, hs, w, gs)
        self.vs, self.ss = [[1, 0, 0], [0, 3, 2]], ss          # election A: race 0 one-hot (S = 1), race 1 a weighted choice (S = 5)
        self.w_b = 21                                          # another election: another key AND another slot width
        nb, gb, hb, gsb, _, _ = _inputs(bits, Rn, K, b, self.w_b, self.s_bits, 0xb132)
        self.elec_b = (nb, gb, hb, self.w_b, gsb)
        assert nb != nn and hb != hs and gsb[1] != pow(gb, 1 << w, nb * nb)
        rng = random.Random(0xb131)
        self.s_tox = rng.randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        shape = dict(count=Rn, slots=K, m_bits=b, s_limbs=sl)
        self.ns = prover_native.NativeStructure(eng, "pballot", bits, W, lb, k, expose=True, **shape)
        self.sa = CS.stream_structure("pballot", bits, W, lb, **shape)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)
        self.structure = self.ns.download()

    def trace(self, elec=None, vs=None, ss=None, forge=None):
        nn, g, hs, w, gs = self.elec_a if elec is None else elec
        return BR.pballot_trace(nn, hs, gs, self.vs if vs is None else vs, self.ss if ss is None else ss, self.b, self.s_bits, forge=forge)

    def statement(self, trace, elec=None, res=None):
        nn, g, hs, w, gs = self.elec_a if elec is None else elec
        return BR.statement(nn, hs, gs, trace.cts if res is None else res, trace.totals, self.bits, self.W)

    def _cells(self, elec, vs, ss, tr, res=None):
        nn, g, hs, w, gs = elec
        return BR.pballot_cells(nn, hs, gs, vs, ss, tr.cts if res is None else res, self.b, self.sl, self.bits, self.W, self.lb, tr)

    def witness(self, elec=None, vs=None, ss=None, trace=None, res=None):
        """K4's columns [m'][2^k][4] from K3's records (trace = None) or from a given trace (the forged ones).  K4 reads the chains' bits
        and forms the sums from `inputs`: a forged chain's num_to_bits must hold the exponent it was run with, so a forged trace is
        expanded from its exponents, and the load_witness, sum and assign_integer(s_i) cells (with the lookup cells of the latter) are
        then put back to the reference's (the values; S_i + delta; the s_i).  res: the claimed ciphertexts (default: the trace's)"""
        import torch

        eng, cref, ns = self.eng, self.cref, self.ns
        elec = self.elec_a if elec is None else elec
        nn, g, hs, w, gs = elec
        vs = self.vs if vs is None else vs
        ss = self.ss if ss is None else ss
        tr = self.trace(elec, vs, ss) if trace is None else trace
        d_steps = _device_records(eng, cref, self.bits, nn, hs, gs, vs, ss, self.b, self.s_bits, trace)
        d_mod = torch.from_numpy(cref.int_to_limbs(nn ** 2, _words(2 * self.bits)).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        eng.pballot_expand_cols_dev(self.bits // self.W, self.W, self.lb, self.R, self.K, self.b, self.sl,
                                    _pballot_inputs(cref, self.bits, self.s_bits, nn, hs, gs, tr.v_exps, tr.s_exps, tr.cts if res is None else res),
                                    d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv,
                                    ns.max_rows, ns.max_rows, self.n_rows)
        eng.sync()
        if trace is not None:
            want_a, want_l, seg = self._cells(elec, vs, ss, tr, res)
            mont = lambda v: torch.from_numpy(cref.fr_ints_to_mont([v])[0].astype(np.int64)).cuda()
            lo, hi = seg["values"][0], seg["square"][0]
            assert hi < int(ns.starts()[1])                  # the head of the stream lies in column 0
            for c in range(lo, hi):
                cols[0, c] = mont(want_a[c])
            llo, lhi = seg["assign_ss"][1], seg["refresh"][1]
            assert lhi < ns.max_rows                          # ... and its lookups in the first lookup column
            for c in range(llo, lhi):
                cols[ns.n_adv, c] = mont(want_l[c])
        return cols

    def reference_columns(self, elec, vs, ss, trace, res=None):
        want_a, want_l, _ = self._cells(elec, vs, ss, trace, res)
        return BR.place(want_a, want_l, self.ns.starts(), self.ns.n_adv, self.ns.n_lk, self.ns.max_rows, self.k, [])

    def ints(self, cols):
        host = cols.cpu().numpy().view(np.uint64)
        return [self.cref.fr_mont_to_ints(host[j]) for j in range(self.ns.m)]

    def check(self, ints, instances):
        """tally_ref.check_columns on a device-written witness under the NATIVE structure"""
        ns = self.ns
        sel, mc, mr = self.structure
        ck = ns.n_adv + ns.n_lk
        ints = list(ints)
        ints[ck] = [c % R for c in ns.constants()] + ints[ck][ns.n_constants:]
        ints[ck + 1] = list(instances) + ints[ck + 1][len(instances):]
        return BR.check_columns(sel, mc, mr, range(1 << self.lb), ints, ns.n_lk)

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
    assert inst == w.statement(tr) and len(inst) == 2 + 4 * (1 + 3 + 2) + 2 and inst[-2:] == [1, 5]
    assert w.check(w.ints(cols), inst) == []
    assert w.ns.n_adv_used >= 20                            # break points are crossed inside every chain
    # the two keys describe one circuit
    a, b = w.key.vk_commitments(), w.pk.vk_commitments()
    assert np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])


def test_connected_proof_both_provers_two_elections_one_key(eng, cref, world):
    """two ballot papers under different n, g, hs AND slot width are proven under ONE proving key and verified under ONE verifying key:
    neither the key nor w enters the circuit's shape"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    tr_a = w.trace()
    vs_b, ss_b = [[0, 2, 1], [3, 3, 3]], [w.ss[1] ^ 5, (1 << w.s_bits) - 3]
    tr_b = w.trace(w.elec_b, vs_b, ss_b)
    good, other = w.statement(tr_a), w.statement(tr_b, w.elec_b)
    kw = dict(enc_bits=w.bits, limb_bits=w.W, slots=w.K, m_bits=w.b)
    (na, ga, ha, wa, _), (nb, gb, hb, wb, _) = w.elec_a, w.elec_b
    assert PV.public_inputs("pballot", n=na, g=ga, hs=ha, slot_bits=wa, cts=tr_a.cts, totals=[1, 5], **kw) == good
    assert PV.public_inputs("pballot", n=nb, g=gb, hs=hb, slot_bits=wb, cts=tr_b.cts, totals=[3, 9], **kw) == other != good
    seeds = [b"pballot-stepper", b"pballot-python", b"pballot-second"]
    cols = w.witness()
    p0 = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seeds[0]), seed=5, instances=good)
    p1 = prover.create_proof(w.pk, w.witness(), prover.HashTranscript(seeds[1]), seed=6, tile=8, instances=good)
    cols2 = w.witness(w.elec_b, vs_b, ss_b)
    assert w.ns.gather_public(cols2.data_ptr()) == other
    assert w.check(w.ints(cols2), other) == []
    p2 = prover_native.create_proof(w.key, cols2.data_ptr(), prover.HashTranscript(seeds[2]), seed=7, instances=other)       # the SAME key
    proofs, inst = [p0, p1, p2], [good, good, other]
    for pr, seed, st in zip(proofs, seeds, inst):
        assert _oracle_checks(cref, w, pr, seed, st) == (True, True, True)
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])          # pz_verify_batch_pub
    wire = [PV.proof_to_bytes(eng, w.vk, p) for p in proofs]
    assert PV.verify_batch_bytes(eng, w.params, w.vk, wire, seeds, instances=inst) == (True, [True, True, True])
    # election A's proofs under election B's statement; under their own with the last total + 1; under A's key read with B's slot width
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[other, other, other]) == (False, [False, False, True])
    plus = list(good)
    plus[-1] += 1
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[plus, plus, other]) == (False, [False, False, True])
    wrong_w = PV.public_inputs("pballot", n=na, g=ga, hs=ha, slot_bits=wb, cts=tr_a.cts, totals=[1, 5], **kw)
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[wrong_w, wrong_w, other]) == (False, [False, False, True])


# (ciphertext 0 is one-hot in slot 0; ciphertext 1 holds 0, 3, 2)
FORGES = [("val", 1, 1, 1), ("base", 0, 0, 1), ("swap", 0), ("fold", 1, 0, 1), ("sum", 1, 1), ("s", 0, 5), ("final", 1)]
FORGE_IDS = ["slot-chain-run-with-another-value", "slot-chain-first-sq-is-G+1", "slot-0-chain-on-G1", "fold-operand-is-P+1", "sum-is-S+1",
             "s-chain-run-with-another-s", "final-result"]


@pytest.mark.parametrize("forge", FORGES, ids=FORGE_IDS)
def test_forged_edges_are_rejected(eng, cref, world, forge):
    """slot chain (1, 1) run consistently with v' = 1 while its load_witness cell (and the sum) says 3; slot chain (0, 0)'s first sq
    taken as G_0 + 1; slot 0's chain of ciphertext 0 run on G_1 (the base swap: the vote moves to candidate 1); fold 0 of ciphertext 1
    fed P_1 + 1; the last cell of ciphertext 1's sum S + 1; hs-chain 0 run with s' = 5 while assign_integer(s_0) keeps s_0; a claimed
    ciphertext that is not the last fold's remainder -- each with everything downstream, the claimed ciphertexts and the statement
    recomputed consistently, expanded through the DEVICE K4 from the forged records.  Every lookup holds; a copy constraint objects
    (the sum: its own gate).  For two cheap ones a proof made from the forged witness is refused."""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    honest = w.trace()
    res = None
    if forge[0] == "final":
        ft = honest
        res = [honest.cts[0], honest.cts[1] ^ 2]
    else:
        ft = w.trace(forge=forge)
        assert (ft.cts != honest.cts) == (forge[0] != "sum")
    inst = w.statement(ft, res=res)
    cols = w.witness(trace=ft, res=res)
    ints = w.ints(cols)
    ref = w.reference_columns(w.elec_a, w.vs, w.ss, ft, res)
    for j in range(w.ns.n_adv + w.ns.n_lk):
        assert ints[j] == ref[j], j
    assert w.ns.gather_public(cols.data_ptr()) == inst
    bad = w.check(ints, inst)
    assert bad and {t for t, _, _ in bad} == ({"gate"} if forge[0] == "sum" else {"copy"})
    if forge[0] in ("swap", "sum"):
        seed = b"pballot-forged"
        hinst = w.statement(honest)
        pf = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=inst)
        ph = prover_native.create_proof(w.key, w.witness().data_ptr(), prover.HashTranscript(seed), seed=9, instances=hinst)
        assert not pf.h_degree_ok and ph.h_degree_ok
        assert PV.verify_batch_native(eng, w.params, w.vk, [pf, ph], [seed, seed], instances=[inst, hinst]) == (False, [False, True])


def test_five_voters_tally_decrypt_and_unpack_to_the_counts(eng, cref):
    """value level, end to end: hs and the slot bases from the device, five voters' one-hot packed ballots in ONE pz_paillier_pballot
    call, pz_paillier_tally of the five, pz_paillier_decrypt of the product, keys.unpack_tally: the per-candidate counts"""
    from paillier_halo2_amd import keys
    from tests import decrypt_ref as DR

    bits, K, w, b, s_bits = 128, 4, 8, 1, 100
    key = DR.key(bits)
    n, g = key[0], key[1]
    Ln = _words(bits)
    rng = random.Random(0xb140)
    x = _unit(rng, n)
    hs = keys.djn_generator(eng, n, rand=lambda k_: x)
    gs = keys.pballot_bases(eng, n, g, K, w)
    assert gs == BR.bases(n, g, K, w)
    choices = [2, 0, 2, 3, 2]
    assert len(choices) <= keys.pballot_capacity(w, b)
    vs = [[int(j == ch) for j in range(K)] for ch in choices]
    ss = [rng.randrange(1 << s_bits) for _ in choices]
    c, _ = _k3(eng, cref, bits, n, hs, gs, vs, ss, b, s_bits, want_steps=False)
    h = BR.djn_h(n, x)
    assert [cref.limbs_to_int(row) for row in c] == [P.paillier_enc_native(n, g, keys.pack_choices(row, w), pow(h, s, n)) for row, s in zip(vs, ss)]
    prod, _ = eng.paillier_tally(Ln, cref.int_to_limbs(n, Ln), c, want_steps=False)
    sk = eng.paillier_sk(Ln, n, g, key[2], key[3])
    try:
        m_, _, fl = eng.paillier_decrypt(sk, prod.reshape(1, -1), want_r=False)
        assert fl.tolist() == [0]
        assert keys.unpack_tally(cref.limbs_to_int(m_[0]), K, w) == [1, 0, 3, 1]
        m1, r1, fl1 = eng.paillier_decrypt(sk, c[:1])
        assert fl1.tolist() == [0] and cref.limbs_to_int(m1[0]) == 1 << (2 * w) and cref.limbs_to_int(r1[0]) == pow(h, ss[0], n)
    finally:
        sk.free()
