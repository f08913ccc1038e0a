"""GPU: the short-randomness ballot (kind 9 / "sballot") through every layer -- the entries' two chains (K3),
the cell stream (K4), the native structure generator, and connected proofs with the statement "these K ciphertexts are g^m_i hs^s_i
under (n, g, hs) with every m_i below 2^b and every s_i below 2^s_bits, and the m_i add up to S" by both provers, two ballots under
DIFFERENT keys proven with ONE proving key -- against the independent restatement of tests/sballot_ref.py in Python integers.  Every
comparison is exact.

Main shape SS1: 128-bit n, 64-bit limbs, lookup_bits 13, k = 14, K = 3, b = 2, s_limbs = 2 -- an odd K with two sum gates, an s that
crosses a limb, break points crossed inside the chains, 21 public values."""
import math
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import public_ref as PR
from tests import sballot_ref as SR

pytestmark = pytest.mark.gpu

R = P.FR_R
BF = 6
SS1 = (128, 64, 13, 14, 3, 2, 2)
SS2 = (264, 88, 11, 14, 2, 1, 1)       # the reference's add-test key size on 88-bit limbs: K3's fields are repacked
SS3 = (128, 64, 10, 13, 1, 1, 1)       # one ciphertext: no sum, no S


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


def _inputs(bits, K, b, s_bits, seed):
    """messages: 0, 2^b - 1 and a lone top bit where K allows, random below 2^b otherwise; s: the same three of s_bits bits in another
    order, then random"""
    rng = random.Random(seed)
    n, g = P.synth_paillier_inputs(bits, seed)[:2]
    hs = SR.djn_hs(n, _unit(rng, n))
    ms = [_specials(b)[i] if i < 3 else rng.randrange(1 << b) for i in range(K)]
    ss = [_specials(s_bits)[(i + 1) % 3] if i < 3 else rng.randrange(1 << s_bits) for i in range(K)]
    return n, g, hs, ms, ss


def _words(bits):
    return -(-bits // 64)


def _u64(ws):
    return np.array([int(w) for w in ws], dtype=np.uint64)


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


def _k3(eng, cref, bits, n, g, hs, ms, ss, b, s_bits, want_steps=True):
    Ln = _words(bits)
    lim = cref.int_to_limbs
    return eng.paillier_sballot(Ln, lim(n, Ln), lim(g, Ln), lim(hs, 2 * Ln), _u64(ms), np.stack([lim(s, _words(s_bits)) for s in ss]), b, s_bits,
                                want_steps=want_steps)


# ------------------------------------------------------------------------------------------------------------------ 1. K3
K3_SHAPES = [(128, 1, 1, 1), (128, 1, 64, 64), (128, 3, 2, 128), (128, 300, 1, 65), (264, 2, 5, 88), (2048, 2, 3, 130), (3072, 1, 2, 64)]


@pytest.mark.parametrize("bits,K,b,s_bits", K3_SHAPES)
def test_k3_records_equal_the_reference(eng, cref, bits, K, b, s_bits):
    n, g, hs, ms, ss = _inputs(bits, K, b, s_bits, 0x5c20 + 64 * K + b + s_bits)
    vectors = [(ms, ss)]
    if K == 1:      # one entry carries one message and one s: zero, all ones, the lone top bit and a random s each get a run
        rng = random.Random(bits + b + s_bits)
        sm, sv = _specials(b), _specials(s_bits)
        vectors = [([sm[0]], [sv[0]]), ([sm[1]], [sv[1]]), ([sm[2]], [sv[2]]), ([rng.randrange(1 << b)], [rng.randrange(1 << s_bits)])]
    if bits > 2048:
        vectors = vectors[1:2]
    L = 2 * _words(bits)
    per = SR.per_entry(b, s_bits)
    n2 = n * n
    for mv, sv in vectors:
        c, steps = _k3(eng, cref, bits, n, g, hs, mv, sv, b, s_bits)
        tr = SR.sballot_trace(n, g, hs, mv, sv, b, s_bits)
        want = SR.records(tr)
        assert steps.shape == (K, per, 4, L) and len(want) == K * per
        assert [cref.limbs_to_int(row) for row in c] == tr.cts == [pow(g, m, n2) * pow(hs, s, n2) % n2 for m, s in zip(mv, sv)]
        flat = steps.reshape(-1, 4, L)
        want_arr = np.stack([np.stack([cref.int_to_limbs(v, L) for v in st]) for st in want])
        bad = np.nonzero((flat != want_arr).any(axis=(1, 2)))[0]
        assert bad.size == 0, "record %d differs" % bad[0]
        c2, none = _k3(eng, cref, bits, n, g, hs, mv, sv, b, s_bits, want_steps=False)
        assert none is None and np.array_equal(c2, c)


def test_k3_chains_equal_the_parents_kernels_bit_for_bit(eng, cref):
    """an entry's hs-chain is chain 0 of pz_paillier_partial with v = hs, theta = s_i, e_bits = s_bits; its g-chain is
    pz_paillier_ballot's g-chain on the same m_i"""
    bits, K, b, s_bits = 128, 3, 2, 70
    n, g, hs, ms, ss = _inputs(bits, K, b, s_bits, 0x5c21)
    Ln = _words(bits)
    lim = cref.int_to_limbs
    c, steps = _k3(eng, cref, bits, n, g, hs, ms, ss, b, s_bits)
    some_ct = np.stack([lim(hs, 2 * Ln)])
    for i in range(K):
        h, _, prec = eng.paillier_partial(Ln, lim(n, Ln), lim(hs, 2 * Ln), lim(ss[i], 2 * Ln), some_ct, s_bits)
        assert np.array_equal(prec[1:1 + 2 * s_bits], steps[i, 2 * b:2 * b + 2 * s_bits])
        assert cref.limbs_to_int(h) == pow(hs, ss[i], n * n)
    _, bsteps, nr = eng.paillier_ballot(Ln, lim(n, Ln), lim(g, Ln), _u64(ms), np.stack([lim(7 + i, Ln) for i in range(K)]), b)
    assert bsteps.shape[1] == 2 * b + nr + 1
    assert np.array_equal(bsteps[:, :2 * b], steps[:, :2 * b])


def test_k3_refusals_in_their_order(eng, cref):
    from paillier_halo2_amd import _lib

    bits, K, b, s_bits = 128, 3, 2, 65
    n, g, hs, ms, ss = _inputs(bits, K, b, s_bits, 0x5c22)
    lim = cref.int_to_limbs
    sw = _words(s_bits)
    n_, g_, h_, m_, s_ = lim(n, 2), lim(g, 2), lim(hs, 4), _u64(ms), np.stack([lim(s, sw) for s in ss])
    zero_n = lim(0, 2)
    m_bad = _u64([1 << b, 0, 0])                                  # a message of exactly 2^b
    s_bad = np.stack([lim(s, sw) for s in [ss[0], 1 << s_bits, ss[2]]])     # an s of exactly 2^s_bits: bit 1 of its second word
    per = SR.per_entry(b, s_bits)
    need = K * per
    steps = np.zeros((need, 4, 4), dtype=np.uint64)
    out = np.zeros((K, 4), dtype=np.uint64)

    def call(limbs=2, count=K, mb=b, sb=s_bits, nn=n_, hh=h_, mm=m_, sv=s_, cap=need, st=steps, o=out, gg=g_):
        ptr = lambda a: None if a is None else a.ctypes.data
        return eng.L.pz_paillier_sballot(eng.ctx, limbs, count, mb, sb, ptr(nn), ptr(gg), ptr(hh), ptr(mm), ptr(sv), ptr(st), cap, ptr(o))

    # 1. PZ_ERR_INVALID, ahead of everything else (here together with what the later checks would refuse)
    for kw in (dict(nn=None), dict(gg=None), dict(hh=None), dict(mm=None), dict(sv=None), dict(o=None), dict(limbs=0), dict(count=0),
               dict(count=1025), dict(mb=0), dict(mb=65), dict(sb=0), dict(sb=128 * 2 + 1)):
        assert call(**kw) == _lib.PZ_ERR_INVALID, kw
    assert call(limbs=65, count=0, cap=0) == _lib.PZ_ERR_INVALID
    # 2. PZ_ERR_UNSUPPORTED ahead of the capacity (2 * limbs_n > 128: refused before anything is read)
    assert call(limbs=65, cap=0) == _lib.PZ_ERR_UNSUPPORTED
    # 3. PZ_ERR_CAPACITY ahead of the ranges
    assert call(cap=need - 1, mm=m_bad, sv=s_bad, nn=zero_n) == _lib.PZ_ERR_CAPACITY
    # 4. PZ_ERR_MESSAGE_RANGE ahead of the zero modulus: a message, then an s
    assert call(mm=m_bad, nn=zero_n) == _lib.PZ_ERR_MESSAGE_RANGE
    assert call(sv=s_bad, nn=zero_n) == _lib.PZ_ERR_MESSAGE_RANGE
    # 5. PZ_ERR_ZERO_MODULUS
    assert call(nn=zero_n) == _lib.PZ_ERR_ZERO_MODULUS
    assert not steps.any() and not out.any()
    # hs >= n^2: PZ_ERR_RANGE from the kernel's range bit, in both forms; nothing is written
    assert call(hh=lim(n * n, 4)) == _lib.PZ_ERR_RANGE
    assert call(hh=lim(n * n, 4), st=None, cap=0) == _lib.PZ_ERR_RANGE
    assert not steps.any() and not out.any()
    import torch

    d_steps = torch.zeros((need, 4, 4), dtype=torch.int64, device="cuda")
    assert _status(lambda: eng.paillier_sballot_dev(2, n_, g_, lim(n * n + 5, 4), m_, s_, b, s_bits, d_steps.data_ptr(), need)) == _lib.PZ_ERR_RANGE
    assert not bool(d_steps.any())
    # the Engine's wrapper raises the same statuses
    assert _status(lambda: eng.paillier_sballot(2, n_, g_, h_, m_bad, s_, b, s_bits)) == _lib.PZ_ERR_MESSAGE_RANGE
    assert _status(lambda: eng.paillier_sballot(2, n_, g_, h_, m_, s_bad, b, s_bits)) == _lib.PZ_ERR_MESSAGE_RANGE
    # ... and the context serves an honest call afterwards, in both forms
    assert call() == 0
    tr = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits)
    assert [cref.limbs_to_int(row) for row in out] == tr.cts
    assert tuple(cref.limbs_to_int(steps[-1, f]) for f in range(4)) == SR.records(tr)[-1]
    c = eng.paillier_sballot_dev(2, n_, g_, h_, m_, s_, b, s_bits, d_steps.data_ptr(), need)
    assert [cref.limbs_to_int(row) for row in c] == tr.cts
    assert np.array_equal(d_steps.cpu().numpy().view(np.uint64), steps)


# ------------------------------------------------------------------------------------------------------------------ 2. K4
def _device_records(eng, cref, bits, n, g, hs, ms, ss, b, s_bits, trace=None):
    """the K (2 b + 2 s_bits + 1) records on the device AS K3 LEAVES THEM, fields of 2 ceil(bits / 64) words: K3's own (trace = None),
    or a given trace's (the forged ones)"""
    import torch

    rw = 2 * _words(bits)
    lim = cref.int_to_limbs
    if trace is None:
        c, rec = _k3(eng, cref, bits, n, g, hs, ms, ss, b, s_bits)
        assert [cref.limbs_to_int(row) for row in c] == SR.sballot_trace(n, g, hs, ms, ss, b, s_bits).cts
        rec = rec.reshape(-1, 4, rw)
    else:
        rec = np.stack([np.stack([lim(v, rw) for v in st]) for st in SR.records(trace)])
    return torch.from_numpy(np.ascontiguousarray(rec).astype(np.int64)).cuda()


def _sballot_inputs(cref, bits, s_bits, n, g, hs, ms, ss, res):
    lim = cref.int_to_limbs
    wn, wl = _words(bits), _words(2 * bits)
    return np.concatenate([lim(n, wn), lim(g, wn), lim(hs, wl), _u64(ms)] + [lim(s, _words(s_bits)) for s in ss] + [lim(v, wl) for v in res])


@pytest.mark.parametrize("shape", [SS1, SS2, SS3], ids=["SS1", "264-88", "K1"])
def test_k4_dense_stream_and_break_point_columns_equal_the_reference(eng, cref, shape):
    import torch
    from paillier_halo2_amd import _lib, layout

    bits, W, lb, k, K, b, sl = shape
    s_bits = sl * W
    Ln, n_rows = bits // W, 1 << k
    n, g, hs, ms, ss = _inputs(bits, K, b, s_bits, 0x5c23)
    tr = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits)
    want_a, want_l, seg = SR.sballot_cells(n, g, hs, ms, ss, tr.cts, b, sl, bits, W, lb)
    assert seg["satisfied"] and ("sum" in seg) == (K >= 2)
    na, nl = eng.sballot_cells(Ln, W, lb, K, b, sl)
    assert (na, nl) == (len(want_a), len(want_l))
    pub = eng.sballot_public_cells(Ln, W, lb, K, b, sl).tolist()
    assert len(pub) == 2 * Ln + (K + 1) * 2 * Ln + (K >= 2)
    assert [want_a[c] for c in pub] == SR.statement(n, g, hs, tr.cts, sum(ms) if K >= 2 else None, bits, W)
    d_steps = _device_records(eng, cref, bits, n, g, hs, ms, ss, b, s_bits)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    inputs = _sballot_inputs(cref, bits, s_bits, n, g, hs, ms, ss, tr.cts)
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.sballot_expand_dev(Ln, W, lb, K, b, sl, inputs, d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    # ---- the same stream in break-point columns
    rb = layout.row_budget(k)
    starts = layout.break_points(SR.sballot_gate_mask(K, b, sl, bits, W, lb), rb.max_rows)
    A_used = starts.shape[0] - 1
    A, Lk = rb.columns_for(na, filled=A_used), rb.columns_for(nl)
    full = np.concatenate([starts, np.full(A - A_used, na, dtype=np.uint64)])
    d_starts = torch.from_numpy(full.astype(np.int64)).cuda()
    cols = torch.zeros((A + Lk + 1, n_rows, 4), dtype=torch.int64, device="cuda")
    eng.sballot_expand_cols_dev(Ln, W, lb, K, b, sl, inputs, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(), cols[A].data_ptr(),
                                d_starts.data_ptr(), A, rb.max_rows, rb.max_rows, n_rows)
    eng.sync()
    want_cols = SR.place(want_a, want_l, full, A, Lk, rb.max_rows, k, [])
    host = cols.cpu().numpy().view(np.uint64)
    for j in range(A + Lk + 1):
        assert cref.fr_mont_to_ints(host[j]) == want_cols[j], j
    assert A_used >= 2
    # a message that does not fit m_bits and an s that does not fit s_bits are refused by both forms (s_bits = 88: bit 24 of word 1)
    over = [_sballot_inputs(cref, bits, s_bits, n, g, hs, [1 << b] + ms[1:], ss, tr.cts)]
    if s_bits % 64:
        bad_s = _sballot_inputs(cref, bits, s_bits, n, g, hs, ms, ss, tr.cts)
        bad_s[2 * _words(bits) + _words(2 * bits) + K + _words(s_bits) - 1] |= np.uint64(1 << (s_bits % 64))
        over.append(bad_s)
    for inp in over:
        assert _status(lambda: eng.sballot_expand_dev(Ln, W, lb, K, b, sl, inp, d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(),
                                                      d_lk.data_ptr())) == _lib.PZ_ERR_MESSAGE_RANGE
        assert _status(lambda: eng.sballot_expand_cols_dev(Ln, W, lb, K, b, sl, inp, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(),
                                                           cols[A].data_ptr(), d_starts.data_ptr(), A, rb.max_rows, rb.max_rows,
                                                           n_rows)) == _lib.PZ_ERR_MESSAGE_RANGE
    # the by-kind entry points refuse kind 9
    assert _status(lambda: eng.circuit_cells(9, Ln, W, lb, 2 * b, 2 * s_bits)) == _lib.PZ_ERR_INVALID


def test_k4_dense_stream_of_a_mismatching_result_equals_the_reference(eng, cref):
    """entry 1's claimed ciphertext differs from the computed one in a middle limb only, entry 0's matches: the running-equality chain of
    entry 1 drops there and stays down, the is_zero inverse cell of that limb is a true inverse -- the cells the matching streams above
    never reach"""
    import torch

    bits, W, lb, K, b, sl = 128, 64, 10, 2, 2, 1
    s_bits = sl * W
    Ln = bits // W
    n, g, hs, ms, ss = _inputs(bits, K, b, s_bits, 0x5c2a)
    tr = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits)
    res = [tr.cts[0], tr.cts[1] ^ (1 << (W + 5))]       # limb 1 of 4
    want_a, want_l, seg = SR.sballot_cells(n, g, hs, ms, ss, res, b, sl, bits, W, lb)
    assert not seg["satisfied"]
    na, nl = eng.sballot_cells(Ln, W, lb, K, b, sl)
    assert (na, nl) == (len(want_a), len(want_l))
    d_steps = _device_records(eng, cref, bits, n, g, hs, ms, ss, b, s_bits)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.sballot_expand_dev(Ln, W, lb, K, b, sl, _sballot_inputs(cref, bits, s_bits, n, g, hs, ms, ss, res), d_steps.data_ptr(), d_mod.data_ptr(),
                           d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l


# ------------------------------------------------------------------------------------------------------------------ 3. structure
@pytest.mark.parametrize("shape", [SS1, SS3], ids=["SS1", "K1"])
@pytest.mark.parametrize("expose", [False, True])
def test_native_structure_equals_the_python_generator(eng, shape, expose):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout, prover_native

    bits, W, lb, k, K, b, sl = shape
    sa = CS.stream_structure("sballot", bits, W, lb, count=K, m_bits=b, s_limbs=sl)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=expose)
    ns = prover_native.NativeStructure(eng, "sballot", bits, W, lb, k, count=K, m_bits=b, s_limbs=sl, expose=expose)
    try:
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], 2 * b, 2 * sl * W)
        assert ns.starts().tolist() == starts.tolist()
        assert ns.starts()[: ns.n_adv_used + 1].tolist() == layout.break_points(SR.sballot_gate_mask(K, b, sl, bits, W, lb), ns.max_rows).tolist()
        assert ns.constants() == [int(c) for c in cs.constants]
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        Ln = bits // W
        assert (ns.n_instance, ns.n_public) == ((1, 2 * Ln + (K + 1) * 2 * Ln + (K >= 2)) if expose else (0, 0))
        if expose:
            assert ns.public_cells() == cs.public_cells
    finally:
        ns.free()
    for count, m_bits, s_limbs in ((0, b, sl), (1025, b, sl), (K, 0, sl), (K, 65, sl), (K, b, 0), (K, b, 2 * (bits // W) + 1)):
        with pytest.raises(Exception):
            prover_native.NativeStructure(eng, "sballot", bits, W, lb, k, count=count, m_bits=m_bits, s_limbs=s_limbs)


# ------------------------------------------------------------------------------------------------------------------ 4. / 5. the proof
class World:
    """SS1: SRS with a known toxic scalar, both structures with the instance column, both keys -- made from the SHAPE alone, no key of
    an election enters --, witnesses from K3 -> K4"""

    def __init__(self, eng, cref):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.bits, self.W, self.lb, self.k, self.K, self.b, self.sl = SS1
        bits, W, lb, k, K, b, sl = SS1
        self.s_bits = sl * W
        self.n_rows = n = 1 << k
        nn, g, hs, _, ss = _inputs(bits, K, b, self.s_bits, 0x5c30)
        self.key_a = (nn, g, hs)
        self.ms, self.ss = [1, 0, 0], ss                       # ballot A: one-hot (within b = 2 bits), S = 1
        nb, gb, hb, _, _ = _inputs(bits, K, b, self.s_bits, 0x5c32)
        self.key_b = (nb, gb, hb)                              # another election's key
        assert nb != nn and hb != hs
        rng = random.Random(0x5c31)
        self.s_tox = rng.randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        self.ns = prover_native.NativeStructure(eng, "sballot", bits, W, lb, k, count=K, m_bits=b, s_limbs=sl, expose=True)
        self.sa = CS.stream_structure("sballot", bits, W, lb, count=K, m_bits=b, s_limbs=sl)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)
        self.structure = self.ns.download()

    def trace(self, key=None, ms=None, ss=None, forge=None):
        nn, g, hs = self.key_a if key is None else key
        return SR.sballot_trace(nn, g, hs, self.ms if ms is None else ms, self.ss if ss is None else ss, self.b, self.s_bits, forge=forge)

    def statement(self, trace, key=None):
        nn, g, hs = self.key_a if key is None else key
        return SR.statement(nn, g, hs, trace.cts, trace.total, self.bits, self.W)

    def _cells(self, key, ms, ss, tr):
        nn, g, hs = key
        return SR.sballot_cells(nn, g, hs, ms, ss, tr.cts, self.b, self.sl, self.bits, self.W, self.lb, tr)

    def witness(self, key=None, ms=None, ss=None, trace=None):
        """K4's columns [m'][2^k][4] from K3's records (trace = None) or from a given trace (the forged ones).  K4 reads the chains' bits
        and forms the sum from `inputs`: a forged chain's num_to_bits must hold the exponent it was run with, so a forged trace is
        expanded from its exponents, and the load_witness, sum and assign_integer(s_i) cells (with the lookup cells of the latter) are
        then put back to the reference's (the messages; S + delta; the s_i)"""
        import torch

        eng, cref, ns = self.eng, self.cref, self.ns
        key = self.key_a if key is None else key
        nn, g, hs = key
        ms = self.ms if ms is None else ms
        ss = self.ss if ss is None else ss
        tr = self.trace(key, ms, ss) if trace is None else trace
        d_steps = _device_records(eng, cref, self.bits, nn, g, hs, ms, ss, self.b, self.s_bits, trace)
        d_mod = torch.from_numpy(cref.int_to_limbs(nn ** 2, _words(2 * self.bits)).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        eng.sballot_expand_cols_dev(self.bits // self.W, self.W, self.lb, self.K, self.b, self.sl,
                                    _sballot_inputs(cref, self.bits, self.s_bits, nn, g, hs, tr.m_exps, tr.s_exps, tr.cts), d_steps.data_ptr(),
                                    d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows,
                                    self.n_rows)
        eng.sync()
        if trace is not None:
            want_a, want_l, seg = self._cells(key, ms, ss, tr)
            mont = lambda v: torch.from_numpy(cref.fr_ints_to_mont([v])[0].astype(np.int64)).cuda()
            lo, hi = seg["messages"][0], seg["square"][0]
            assert hi < int(ns.starts()[1])                  # the head of the stream lies in column 0
            for c in range(lo, hi):
                cols[0, c] = mont(want_a[c])
            llo, lhi = seg["assign_ss"][1], seg["refresh"][1]
            assert lhi < ns.max_rows                          # ... and its lookups in the first lookup column
            for c in range(llo, lhi):
                cols[ns.n_adv, c] = mont(want_l[c])
        return cols

    def reference_columns(self, key, ms, ss, trace):
        want_a, want_l, _ = self._cells(key, ms, ss, trace)
        return SR.place(want_a, want_l, self.ns.starts(), self.ns.n_adv, self.ns.n_lk, self.ns.max_rows, self.k, [])

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
        return SR.check_columns(sel, mc, mr, range(1 << self.lb), ints, ns.n_lk)

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
    assert inst == w.statement(tr) and len(inst) == 2 * 2 + 4 * 4 + 1 and inst[-1] == 1
    assert w.check(w.ints(cols), inst) == []
    assert w.ns.n_adv_used >= 40                            # break points are crossed inside every chain
    # the two keys describe one circuit
    a, b = w.key.vk_commitments(), w.pk.vk_commitments()
    assert np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])


def test_connected_proof_both_provers_two_elections_one_key(eng, cref, world):
    """two ballots with different n, hs, m and s are proven under ONE proving key and verified under ONE verifying key: the property
    kind 6 cannot have, whose r^n chains carry n's bits in the key's shape"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    tr_a = w.trace()
    ms_b, ss_b = [0, 2, 1], [w.ss[2] ^ 5, 7, (1 << w.s_bits) - 3]
    tr_b = w.trace(w.key_b, ms_b, ss_b)
    good, other = w.statement(tr_a), w.statement(tr_b, w.key_b)
    kw = dict(enc_bits=w.bits, limb_bits=w.W)
    (na, ga, ha), (nb, gb, hb) = w.key_a, w.key_b
    assert PV.public_inputs("sballot", n=na, g=ga, hs=ha, cts=tr_a.cts, total=1, **kw) == good
    assert PV.public_inputs("sballot", n=nb, g=gb, hs=hb, cts=tr_b.cts, total=3, **kw) == other != good
    seeds = [b"sballot-stepper", b"sballot-python", b"sballot-second"]
    cols = w.witness()
    p0 = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seeds[0]), seed=5, instances=good)
    p1 = prover.create_proof(w.pk, w.witness(), prover.HashTranscript(seeds[1]), seed=6, tile=8, instances=good)
    cols2 = w.witness(w.key_b, ms_b, ss_b)
    assert w.ns.gather_public(cols2.data_ptr()) == other
    assert w.check(w.ints(cols2), other) == []
    p2 = prover_native.create_proof(w.key, cols2.data_ptr(), prover.HashTranscript(seeds[2]), seed=7, instances=other)       # the SAME key
    proofs, inst = [p0, p1, p2], [good, good, other]
    for pr, seed, st in zip(proofs, seeds, inst):
        assert _oracle_checks(cref, w, pr, seed, st) == (True, True, True)
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])          # pz_verify_batch_pub
    wire = [PV.proof_to_bytes(eng, w.vk, p) for p in proofs]
    assert PV.verify_batch_bytes(eng, w.params, w.vk, wire, seeds, instances=inst) == (True, [True, True, True])
    # election A's proofs under election B's statement; under their own with total + 1
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[other, other, other]) == (False, [False, False, True])
    plus = list(good)
    plus[-1] += 1
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[plus, plus, other]) == (False, [False, False, True])


FORGES = [("s", 0, 5), ("base", 0, 1), ("msg", 1, 2), ("g", 0, 1), ("final", 0, 1), ("sum", 1)]   # (entry 0 holds the ballot's one set bit)
FORGE_IDS = ["s-chain-run-with-another-s", "s-chain-first-sq-is-hs+1", "g-chain-run-with-another-message", "g-chain-first-sq-is-g+1",
             "final-operand-is-hss+1", "sum-is-S+1"]


@pytest.mark.parametrize("forge", FORGES, ids=FORGE_IDS)
def test_forged_edges_are_rejected(eng, cref, world, forge):
    """hs-chain 0 run consistently with s' = 5 while assign_integer(s_0) keeps s_0; its first sq taken as hs + 1; g-chain 1 run with
    m' = 2 while its load_witness cell (and the sum) says 0; g-chain 0's first sq taken as g + 1; entry 0's final block fed hss + 1; the
    last sum cell S + 1 -- each with everything downstream, the claimed ciphertexts and the statement recomputed consistently, expanded
    through the DEVICE K4 from the forged records.  Every lookup and every final equality holds; a copy constraint objects (the sum:
    its own gate).  For two cheap ones a proof made from the forged witness is refused."""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    ft = w.trace(forge=forge)
    honest = w.trace()
    assert (ft.cts != honest.cts) == (forge[0] != "sum")
    inst = w.statement(ft)
    cols = w.witness(trace=ft)
    ints = w.ints(cols)
    ref = w.reference_columns(w.key_a, w.ms, w.ss, ft)
    for j in range(w.ns.n_adv + w.ns.n_lk):
        assert ints[j] == ref[j], j
    assert w.ns.gather_public(cols.data_ptr()) == inst
    bad = w.check(ints, inst)
    assert bad and {t for t, _, _ in bad} == ({"gate"} if forge[0] == "sum" else {"copy"})
    if forge[0] in ("s", "sum"):
        seed = b"sballot-forged"
        hinst = w.statement(honest)
        pf = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=inst)
        ph = prover_native.create_proof(w.key, w.witness().data_ptr(), prover.HashTranscript(seed), seed=9, instances=hinst)
        assert not pf.h_degree_ok and ph.h_degree_ok
        assert PV.verify_batch_native(eng, w.params, w.vk, [pf, ph], [seed, seed], instances=[inst, hinst]) == (False, [False, True])


def test_sballots_feed_the_tally_and_decrypt_to_the_sum(eng, cref):
    """value level only: hs from keys.djn_generator on the device, the K ciphertexts of pz_paillier_sballot go into pz_paillier_tally,
    and pz_paillier_decrypt of the product returns S; a single ballot decrypts to its message with the randomness h^s mod n"""
    from paillier_halo2_amd import keys
    from tests import decrypt_ref as DR

    bits, K, b, s_bits = 128, 3, 2, 100
    key = DR.key(bits)
    n, g = key[0], key[1]
    Ln = _words(bits)
    rng = random.Random(0x5c40)
    x = _unit(rng, n)
    hs = keys.djn_generator(eng, n, rand=lambda k_: x)
    assert hs == SR.djn_hs(n, x)
    ms = [3, 0, 2]
    ss = [rng.randrange(1 << s_bits) for _ in range(K)]
    c, _ = _k3(eng, cref, bits, n, g, hs, ms, ss, b, s_bits, want_steps=False)
    h = SR.djn_h(n, x)
    assert [cref.limbs_to_int(row) for row in c] == [P.paillier_enc_native(n, g, m, pow(h, s, n)) for m, s in zip(ms, ss)]
    prod, _ = eng.paillier_tally(Ln, cref.int_to_limbs(n, Ln), c, want_steps=False)
    sk = eng.paillier_sk(Ln, n, g, key[2], key[3])
    try:
        m_, _, fl = eng.paillier_decrypt(sk, prod.reshape(1, -1), want_r=False)
        assert fl.tolist() == [0] and cref.limbs_to_int(m_[0]) == sum(ms) == 5
        m1, r1, fl1 = eng.paillier_decrypt(sk, c[:1])
        assert fl1.tolist() == [0] and cref.limbs_to_int(m1[0]) == 3 and cref.limbs_to_int(r1[0]) == pow(h, ss[0], n)
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------------------------ 6. K3 under structured n
# n of 8, 9, 31, 32, 33 and 49 limbs (below, at and past a team's slice boundaries) that are runs of ones and
# zeros, and two Mersenne-product keys, as section 15.13 runs wtally, ballot, encrypt and partial
from tests import k3_operands as KO  # noqa: E402

STRUCT_SHAPES = [(ln, tb) for ln in (8, 9, 31, 32, 33, 49) for tb in (1, 64)] + [("mersenne", 3), ("mersenne", 5)]
STRUCT_B = 2


def _struct_ns(ln, tb):
    if ln == "mersenne":
        p, q = KO.mersenne_primes(tb)
        return KO.words((p * q).bit_length()), [("mersenne%d" % KO.MERSENNE_BITS[tb], p * q)]
    ms = KO.moduli(KO.bits_of(ln, tb))
    return ln, [(cls, ms[cls]) for cls in ("all_ones", "pow2_plus1", "alt32_hi")]


def _bytes_rows(vals, L):
    return np.frombuffer(b"".join(int(v).to_bytes(8 * L, "little") for v in vals), dtype=np.uint64).reshape(len(vals), L).copy()


@pytest.mark.parametrize("ln,tb", STRUCT_SHAPES)
def test_k3_under_structured_n_equals_the_reference(eng, ln, tb):
    """s in {0, all ones, a lone top bit} with m in {0, 2^b - 1}, at s_bits 1, 64 and 65, under hs in {1, n + 1, n^2 - 1, a true h^n};
    hs = n^2 is refused with PZ_ERR_RANGE and nothing is written"""
    from paillier_halo2_amd import _lib

    Ln, cases = _struct_ns(ln, tb)
    L, b = 2 * Ln, STRUCT_B
    for cls, n in cases:
        n2 = n * n
        g = KO.by_name(n, Ln)["alt64"]
        n_, g_ = _bytes_rows([n], Ln)[0], _bytes_rows([g], Ln)[0]
        for hs_name, hs in (("1", 1), ("n+1", n + 1), ("n^2-1", n2 - 1), ("h^n", SR.djn_hs(n, 2))):
            for s_bits in ((65,) if hs_name in ("1", "n+1") else (1, 64, 65)):      # every hs across a limb of s; 1 and 64 bits under two
                ss = list(dict.fromkeys(_specials(s_bits)))
                ms = [[0, (1 << b) - 1][(i + s_bits) % 2] for i in range(len(ss))]      # both messages meet every s over the three widths
                where = (ln, tb, cls, hs_name, s_bits)
                c, steps = eng.paillier_sballot(Ln, n_, g_, _bytes_rows([hs], L)[0], _u64(ms), _bytes_rows(ss, _words(s_bits)), b, s_bits)
                tr = SR.sballot_trace(n, g, hs, ms, ss, b, s_bits)
                want = SR.records(tr)
                assert [int.from_bytes(row.tobytes(), "little") for row in c] == tr.cts == [SR.encrypt(n, g, hs, m, s) for m, s in zip(ms, ss)], where
                want_arr = _bytes_rows([v for st in want for v in st], L).reshape(len(want), 4, L)
                bad = np.nonzero((steps.reshape(-1, 4, L) != want_arr).any(axis=(1, 2)))[0]
                assert bad.size == 0, where + ("record %d differs" % bad[0],)
        # hs of exactly n^2: the kernel's range bit, outputs untouched
        s_bits, K = 65, 2
        per = SR.per_entry(b, s_bits)
        steps = np.full((K * per, 4, L), 0xA5, dtype=np.uint64)
        out = np.full((K, L), 0xA5, dtype=np.uint64)
        h_, m_, s_ = _bytes_rows([n2], L)[0], _u64([1, 2]), _bytes_rows([1, 1 << 64], 2)
        rc = eng.L.pz_paillier_sballot(eng.ctx, Ln, K, b, s_bits, n_.ctypes.data, g_.ctypes.data, h_.ctypes.data, m_.ctypes.data, s_.ctypes.data,
                                       steps.ctypes.data, K * per, out.ctypes.data)
        assert rc == _lib.PZ_ERR_RANGE and (steps == 0xA5).all() and (out == 0xA5).all(), (ln, tb, cls)
