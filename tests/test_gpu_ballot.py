"""GPU: the ballot circuit (kind 6 / "ballot") through every layer -- the entries' chains (K3), the cell stream
(K4), the native structure generator, and ONE connected proof with the statement "these K ciphertexts under (n, g) each hold a value
below 2^b, and the values add up to S" by both provers -- against the independent restatement of tests/ballot_ref.py in Python
integers.  Every comparison is exact.

Main shape SB1: 128-bit n, 64-bit limbs, lookup_bits 13, k = 14, K = 3, b = 2 -- an odd K with two sum gates, break points crossed
inside the chains, 21 public values."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import ballot_ref as BR
from tests import public_ref as PR

pytestmark = pytest.mark.gpu

R = P.FR_R
BF = 6
SB1 = (128, 64, 13, 14, 3, 2)
SB2 = (264, 88, 11, 14, 2, 1)       # the reference's add-test key size on 88-bit limbs
SB3 = (128, 64, 10, 13, 1, 1)       # one ciphertext: no sum, no S


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _inputs(bits, K, b, seed):
    """messages: 0, 2^b - 1 and a lone top bit where K allows, random below 2^b otherwise; r: 1, n - 1, then random"""
    rng = random.Random(seed)
    n, g = P.synth_paillier_inputs(bits, seed)[:2]
    special = [0, (1 << b) - 1, 1 << (b - 1)]
    ms = [special[i] if i < 3 else rng.randrange(1 << b) for i in range(K)]
    rs = [[1, n - 1][i] if i < 2 else rng.randrange(1, n) for i in range(K)]
    return n, g, ms, rs


def _words(bits):
    return -(-bits // 64)


def _u64(ws):
    return np.array([int(w) for w in ws], dtype=np.uint64)


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


def _k3(eng, cref, bits, n, g, ms, rs, b, want_steps=True):
    Ln = _words(bits)
    lim = cref.int_to_limbs
    return eng.paillier_ballot(Ln, lim(n, Ln), lim(g, Ln), _u64(ms), np.stack([lim(r, Ln) for r in rs]), b, want_steps=want_steps)


# ------------------------------------------------------------------------------------------------------------------ 1. K3
K3_SHAPES = [(128, 1, 1), (128, 1, 64), (128, 3, 2), (128, 300, 1), (264, 2, 5), (2048, 2, 3), (3072, 1, 2)]


@pytest.mark.parametrize("bits,K,b", K3_SHAPES)
def test_k3_records_equal_the_reference(eng, cref, bits, K, b):
    n, g, ms, rs = _inputs(bits, K, b, 0x6b20 + 64 * K + b)
    vectors = [(ms, rs)]
    if K == 1:      # one entry carries one message: zero, all ones and the lone top bit each get a run, with r = 1, n - 1, random
        vectors = [([0], [1]), ([(1 << b) - 1], [n - 1]), ([1 << (b - 1)], [random.Random(bits + b).randrange(1, n)])]
    if bits > 2048:
        vectors = vectors[1:2]
    L = 2 * _words(bits)
    nr = BR.n_steps_r(n)
    for mv, rv in vectors:
        c, steps, got_nr = _k3(eng, cref, bits, n, g, mv, rv, b)
        tr = BR.ballot_trace(n, g, mv, rv, b)
        want = BR.records(tr)
        assert got_nr == nr and steps.shape == (K, 2 * b + nr + 1, 4, L) and len(want) == K * (2 * b + nr + 1)
        assert [cref.limbs_to_int(row) for row in c] == tr.cts == [pow(g, m, n * n) * pow(r, n, n * n) % (n * n) for m, r in zip(mv, rv)]
        flat = steps.reshape(-1, 4, L)
        want_arr = np.stack([np.stack([cref.int_to_limbs(v, L) for v in st]) for st in want])
        bad = np.nonzero((flat != want_arr).any(axis=(1, 2)))[0]
        assert bad.size == 0, "record %d differs" % bad[0]
        c2, none, _ = _k3(eng, cref, bits, n, g, mv, rv, b, want_steps=False)
        assert none is None and np.array_equal(c2, c)


def test_k3_chains_equal_the_uniform_encrypt_records(eng, cref):
    """the g-chain and r-chain records (and the final one) are what pz_paillier_encrypt_uniform_dev(batch = K, m_bits = b) writes"""
    import torch

    bits, K, b = 128, 3, 2
    n, g, ms, rs = _inputs(bits, K, b, 0x6b21)
    Ln = _words(bits)
    lim = cref.int_to_limbs
    c, steps, nr = _k3(eng, cref, bits, n, g, ms, rs, b)
    per = 2 * b + nr + 1
    d_steps = torch.zeros((K, per, 4, 2 * Ln), dtype=torch.int64, device="cuda")
    rep = lambda v: np.stack([lim(v, Ln)] * K)
    cu, ng_u, nr_u = eng.paillier_encrypt_uniform_dev(Ln, b, rep(n), rep(g), np.stack([lim(m, Ln) for m in ms]), np.stack([lim(r, Ln) for r in rs]),
                                                      d_steps.data_ptr(), per)
    assert ng_u.tolist() == [2 * b] * K and nr_u.tolist() == [nr] * K and np.array_equal(cu, c)
    assert np.array_equal(d_steps.cpu().numpy().view(np.uint64), steps)


def test_k3_refusals(eng, cref):
    from paillier_halo2_amd import _lib

    bits, K, b = 128, 3, 2
    n, g, ms, rs = _inputs(bits, K, b, 0x6b22)
    lim = cref.int_to_limbs
    n_, g_, m_, r_ = lim(n, 2), lim(g, 2), _u64(ms), np.stack([lim(r, 2) for r in rs])
    assert _status(lambda: eng.paillier_ballot(2, n_, g_, _u64([0, 4, 1]), r_, b)) == _lib.PZ_ERR_MESSAGE_RANGE       # 4 = 2^b
    assert _status(lambda: eng.paillier_ballot(2, n_, g_, m_, r_, 0)) == _lib.PZ_ERR_INVALID
    assert _status(lambda: eng.paillier_ballot(2, n_, g_, m_, r_, 65)) == _lib.PZ_ERR_INVALID
    assert _status(lambda: eng.paillier_ballot(2, lim(0, 2), g_, m_, r_, b)) == _lib.PZ_ERR_ZERO_MODULUS
    nr = BR.n_steps_r(n)
    need = K * (2 * b + nr + 1)
    steps = np.zeros((need, 4, 4), dtype=np.uint64)
    out = np.zeros((K, 4), dtype=np.uint64)
    call = lambda limbs, count, cap: eng.L.pz_paillier_ballot(eng.ctx, limbs, count, b, n_.ctypes.data, g_.ctypes.data, m_.ctypes.data,
                                                              r_.ctypes.data, steps.ctypes.data, cap, None, out.ctypes.data)
    assert call(2, 0, need) == _lib.PZ_ERR_INVALID
    assert call(2, 1025, need) == _lib.PZ_ERR_INVALID
    assert call(2, K, need - 1) == _lib.PZ_ERR_CAPACITY
    assert call(65, K, need) == _lib.PZ_ERR_UNSUPPORTED                    # 2 * limbs_n > 128 (refused before anything is read)
    # a message of exactly 2^b is refused before any launch: nothing was written, and the context serves an honest call
    steps[:] = 0
    m_bad = _u64([1 << b, 0, 0])
    assert eng.L.pz_paillier_ballot(eng.ctx, 2, K, b, n_.ctypes.data, g_.ctypes.data, m_bad.ctypes.data, r_.ctypes.data, steps.ctypes.data, need,
                                    None, out.ctypes.data) == _lib.PZ_ERR_MESSAGE_RANGE
    assert not steps.any() and not out.any()
    assert call(2, K, need) == 0
    tr = BR.ballot_trace(n, g, ms, rs, b)
    assert [cref.limbs_to_int(row) for row in out] == tr.cts
    assert tuple(cref.limbs_to_int(steps[-1, f]) for f in range(4)) == BR.records(tr)[-1]


# ------------------------------------------------------------------------------------------------------------------ 2. K4
def _device_records(eng, cref, bits, n, g, ms, rs, b, trace=None):
    """the K (2 b + nr + 1) records on the device, fields of ceil(2 bits / 64) words: K3's own (trace = None), or a given trace's (the
    forged ones)"""
    import torch

    L64 = _words(2 * bits)
    lim = cref.int_to_limbs
    if trace is None:
        c, rec, _ = _k3(eng, cref, bits, n, g, ms, rs, b)
        assert [cref.limbs_to_int(row) for row in c] == BR.ballot_trace(n, g, ms, rs, b).cts
        rec = rec.reshape(-1, 4, rec.shape[-1])
        assert not rec[:, :, L64:].any()
        rec = np.ascontiguousarray(rec[:, :, :L64])      # (264-bit n on 88-bit limbs: K3 writes 10 words a field, K4 reads 9)
    else:
        rec = np.stack([np.stack([lim(v, L64) for v in st]) for st in BR.records(trace)])
    return torch.from_numpy(rec.astype(np.int64)).cuda()


def _ballot_inputs(cref, bits, n, g, ms, rs, res):
    lim = cref.int_to_limbs
    wn, wl = _words(bits), _words(2 * bits)
    return np.concatenate([lim(n, wn), lim(g, wn), _u64(ms)] + [lim(r, wn) for r in rs] + [lim(v, wl) for v in res])


@pytest.mark.parametrize("shape", [SB1, SB2, SB3], ids=["SB1", "264-88", "K1"])
def test_k4_dense_stream_and_break_point_columns_equal_the_reference(eng, cref, shape):
    import torch
    from paillier_halo2_amd import layout

    bits, W, lb, k, K, b = shape
    Ln, n_rows = bits // W, 1 << k
    n, g, ms, rs = _inputs(bits, K, b, 0x6b23)
    tr = BR.ballot_trace(n, g, ms, rs, b)
    nr = BR.n_steps_r(n)
    want_a, want_l, seg = BR.ballot_cells(n, g, ms, rs, tr.cts, b, bits, W, lb)
    assert seg["satisfied"] and ("sum" in seg) == (K >= 2)
    na, nl = eng.ballot_cells(Ln, W, lb, K, b, nr)
    assert (na, nl) == (len(want_a), len(want_l))
    pub = eng.ballot_public_cells(Ln, W, lb, K, b, nr).tolist()
    assert len(pub) == 2 * Ln + K * 2 * Ln + (K >= 2)
    assert [want_a[c] for c in pub] == BR.statement(n, g, tr.cts, sum(ms) if K >= 2 else None, bits, W)
    d_steps = _device_records(eng, cref, bits, n, g, ms, rs, b)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    inputs = _ballot_inputs(cref, bits, n, g, ms, rs, tr.cts)
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.ballot_expand_dev(Ln, W, lb, K, b, nr, inputs, d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    # ---- the same stream in break-point columns
    rb = layout.row_budget(k)
    starts = layout.break_points(BR.ballot_gate_mask(K, b, bits, W, lb, nr), rb.max_rows)
    A_used = starts.shape[0] - 1
    A, Lk = rb.columns_for(na, filled=A_used), rb.columns_for(nl)
    full = np.concatenate([starts, np.full(A - A_used, na, dtype=np.uint64)])
    d_starts = torch.from_numpy(full.astype(np.int64)).cuda()
    cols = torch.zeros((A + Lk + 1, n_rows, 4), dtype=torch.int64, device="cuda")
    eng.ballot_expand_cols_dev(Ln, W, lb, K, b, nr, inputs, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(), cols[A].data_ptr(),
                               d_starts.data_ptr(), A, rb.max_rows, rb.max_rows, n_rows)
    eng.sync()
    want_cols = BR.place(want_a, want_l, full, A, Lk, rb.max_rows, k, [])
    host = cols.cpu().numpy().view(np.uint64)
    for j in range(A + Lk + 1):
        assert cref.fr_mont_to_ints(host[j]) == want_cols[j], j
    assert A_used >= 2
    # a message that does not fit m_bits is refused by both forms
    from paillier_halo2_amd import _lib

    over = _ballot_inputs(cref, bits, n, g, [1 << b] + ms[1:], rs, tr.cts)
    assert _status(lambda: eng.ballot_expand_dev(Ln, W, lb, K, b, nr, over, d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(),
                                                 d_lk.data_ptr())) == _lib.PZ_ERR_MESSAGE_RANGE
    assert _status(lambda: eng.ballot_expand_cols_dev(Ln, W, lb, K, b, nr, over, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(),
                                                      cols[A].data_ptr(), d_starts.data_ptr(), A, rb.max_rows, rb.max_rows,
                                                      n_rows)) == _lib.PZ_ERR_MESSAGE_RANGE
    # the by-kind entry points keep refusing kind 6
    assert _status(lambda: eng.circuit_cells(6, Ln, W, lb, 2 * b, nr)) == _lib.PZ_ERR_INVALID


def test_k4_dense_stream_of_a_mismatching_result_equals_the_reference(eng, cref):
    """entry 1's claimed ciphertext differs from the computed one in a middle limb only, entry 0's matches: the running-equality chain of
    entry 1 drops there and stays down, the is_zero inverse cell of that limb is a true inverse -- the cells the matching streams above
    never reach"""
    import torch

    bits, W, lb, K, b = 128, 64, 10, 2, 2
    Ln = bits // W
    n, g, ms, rs = _inputs(bits, K, b, 0x6b2a)
    tr = BR.ballot_trace(n, g, ms, rs, b)
    nr = BR.n_steps_r(n)
    res = [tr.cts[0], tr.cts[1] ^ (1 << (W + 5))]       # limb 1 of 4
    want_a, want_l, seg = BR.ballot_cells(n, g, ms, rs, res, b, bits, W, lb)
    assert not seg["satisfied"]
    na, nl = eng.ballot_cells(Ln, W, lb, K, b, nr)
    assert (na, nl) == (len(want_a), len(want_l))
    d_steps = _device_records(eng, cref, bits, n, g, ms, rs, b)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.ballot_expand_dev(Ln, W, lb, K, b, nr, _ballot_inputs(cref, bits, n, g, ms, rs, res), d_steps.data_ptr(), d_mod.data_ptr(),
                          d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l


# ------------------------------------------------------------------------------------------------------------------ 3. structure
@pytest.mark.parametrize("shape", [SB1, SB3], ids=["SB1", "K1"])
@pytest.mark.parametrize("expose", [False, True])
def test_native_structure_equals_the_python_generator(eng, shape, expose):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout, prover_native

    bits, W, lb, k, K, b = shape
    n = _inputs(bits, K, b, 0x6b24)[0]
    nr = BR.n_steps_r(n)
    sa = CS.stream_structure("ballot", bits, W, lb, exp_r=n, count=K, m_bits=b)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=expose)
    ns = prover_native.NativeStructure(eng, "ballot", bits, W, lb, k, exp_r=n, count=K, m_bits=b, expose=expose)
    try:
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], 2 * b, nr)
        assert ns.starts().tolist() == starts.tolist()
        assert ns.starts()[: ns.n_adv_used + 1].tolist() == layout.break_points(BR.ballot_gate_mask(K, b, bits, W, lb, nr), ns.max_rows).tolist()
        assert ns.constants() == [int(c) for c in cs.constants]
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        Ln = bits // W
        assert (ns.n_instance, ns.n_public) == ((1, 2 * Ln + K * 2 * Ln + (K >= 2)) if expose else (0, 0))
        if expose:
            assert ns.public_cells() == cs.public_cells
    finally:
        ns.free()
    for count, m_bits in ((0, b), (1025, b), (K, 0), (K, 65)):
        with pytest.raises(Exception):
            prover_native.NativeStructure(eng, "ballot", bits, W, lb, k, exp_r=n, count=count, m_bits=m_bits)


# ------------------------------------------------------------------------------------------------------------------ 4. / 5. the proof
class World:
    """SB1: SRS with a known toxic scalar, both structures with the instance column, both keys, witnesses from K3 -> K4"""

    def __init__(self, eng, cref):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.bits, self.W, self.lb, self.k, self.K, self.b = SB1
        bits, W, lb, k, K, b = SB1
        self.n_rows = n = 1 << k
        self.nn, self.g, _, self.rs = _inputs(bits, K, b, 0x6b30)
        self.ms = [1, 0, 0]                                  # ballot A: one-hot (within b = 2 bits), S = 1
        self.nr = BR.n_steps_r(self.nn)
        rng = random.Random(0x6b31)
        self.s_tox = rng.randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        self.ns = prover_native.NativeStructure(eng, "ballot", bits, W, lb, k, exp_r=self.nn, count=K, m_bits=b, expose=True)
        self.sa = CS.stream_structure("ballot", bits, W, lb, exp_r=self.nn, count=K, m_bits=b)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)
        self.structure = self.ns.download()

    def trace(self, ms=None, rs=None, forge=None):
        return BR.ballot_trace(self.nn, self.g, self.ms if ms is None else ms, self.rs if rs is None else rs, self.b, forge=forge)

    def statement(self, trace):
        return BR.statement(self.nn, self.g, trace.cts, trace.total, self.bits, self.W)

    def witness(self, ms=None, rs=None, trace=None):
        """K4's columns [m'][2^k][4] from K3's records (trace = None) or from a given trace (the forged ones).  K4 reads the chains' bits
        and forms the sum from `inputs`: a forged chain's num_to_bits must hold the exponent it was run with, so a forged trace is
        expanded from its exponents, and the load_witness and sum cells are then put back to the reference's (the messages; S + delta)"""
        import torch

        eng, cref, ns = self.eng, self.cref, self.ns
        ms = self.ms if ms is None else ms
        rs = self.rs if rs is None else rs
        tr = self.trace(ms, rs) if trace is None else trace
        d_steps = _device_records(eng, cref, self.bits, self.nn, self.g, ms, rs, self.b, trace)
        d_mod = torch.from_numpy(cref.int_to_limbs(self.nn ** 2, _words(2 * self.bits)).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        eng.ballot_expand_cols_dev(self.bits // self.W, self.W, self.lb, self.K, self.b, self.nr,
                                   _ballot_inputs(cref, self.bits, self.nn, self.g, tr.exponents, rs, tr.cts), d_steps.data_ptr(),
                                   d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows,
                                   self.n_rows)
        eng.sync()
        if trace is not None:
            want_a, _, seg = BR.ballot_cells(self.nn, self.g, ms, rs, tr.cts, self.b, self.bits, self.W, self.lb, tr)
            lo, hi = seg["messages"][0], seg["assign_rs"][0]
            assert hi < int(ns.starts()[1])                  # the head of the stream lies in column 0
            for c in range(lo, hi):
                cols[0, c] = torch.from_numpy(cref.fr_ints_to_mont([want_a[c]])[0].astype(np.int64)).cuda()
        return cols

    def reference_columns(self, ms, rs, trace):
        want_a, want_l, _ = BR.ballot_cells(self.nn, self.g, ms, rs, trace.cts, self.b, self.bits, self.W, self.lb, trace)
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
    assert inst == w.statement(tr) and len(inst) == 2 * 2 + 3 * 4 + 1 and inst[-1] == 1
    assert w.check(w.ints(cols), inst) == []
    assert w.ns.n_adv_used >= 40                            # break points are crossed inside every chain
    # the two keys describe one circuit
    a, b = w.key.vk_commitments(), w.pk.vk_commitments()
    assert np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])


def test_connected_proof_both_provers_two_ballots_one_key(eng, cref, world):
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    tr_a = w.trace()
    ms_b, rs_b = [0, 2, 1], [w.rs[2], 7, w.rs[1]]
    tr_b = w.trace(ms_b, rs_b)
    good, other = w.statement(tr_a), w.statement(tr_b)
    kw = dict(enc_bits=w.bits, limb_bits=w.W)
    assert PV.public_inputs("ballot", n=w.nn, g=w.g, cts=tr_a.cts, total=1, **kw) == good
    assert PV.public_inputs("ballot", n=w.nn, g=w.g, cts=tr_b.cts, total=3, **kw) == other != good
    seeds = [b"ballot-stepper", b"ballot-python", b"ballot-second"]
    cols = w.witness()
    p0 = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seeds[0]), seed=5, instances=good)
    p1 = prover.create_proof(w.pk, w.witness(), prover.HashTranscript(seeds[1]), seed=6, tile=8, instances=good)
    cols2 = w.witness(ms_b, rs_b)
    assert w.ns.gather_public(cols2.data_ptr()) == other
    p2 = prover_native.create_proof(w.key, cols2.data_ptr(), prover.HashTranscript(seeds[2]), seed=7, instances=other)       # the SAME key
    proofs, inst = [p0, p1, p2], [good, good, other]
    for pr, seed, st in zip(proofs, seeds, inst):
        assert _oracle_checks(cref, w, pr, seed, st) == (True, True, True)
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])          # pz_verify_batch_pub
    wire = [PV.proof_to_bytes(eng, w.vk, p) for p in proofs]
    assert PV.verify_batch_bytes(eng, w.params, w.vk, wire, seeds, instances=inst) == (True, [True, True, True])
    # ballot A's proofs under ballot B's statement; under its own with total + 1
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[other, other, other]) == (False, [False, False, True])
    plus = list(good)
    plus[-1] += 1
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[plus, plus, other]) == (False, [False, False, True])


FORGES = [("exp", 1, 2), ("base", 0, 1), ("rn", 0, 1), ("sum", 1)]      # (chain 1 holds the ballot's one set bit: its base matters)


@pytest.mark.parametrize("forge", FORGES, ids=["chain-run-with-another-message", "first-sq-is-g+1", "final-operand-is-rn+1", "sum-is-S+1"])
def test_forged_edges_are_rejected(eng, cref, world, forge):
    """chain 2 run consistently with m' = 2 while its load_witness cell (and the sum) says 0; chain 1's first sq taken as g + 1; entry
    1's final block fed rn + 1; the last sum cell S + 1 -- each with everything downstream, the claimed ciphertexts and the statement
    recomputed consistently, expanded through the DEVICE K4 from the forged records.  Every lookup and every final equality holds; a
    copy constraint objects (the sum: its own gate).  For the two cheap ones a proof made from the forged witness is refused."""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    ft = w.trace(forge=forge)
    honest = w.trace()
    assert (ft.cts != honest.cts) == (forge[0] != "sum")
    inst = w.statement(ft)
    cols = w.witness(trace=ft)
    ints = w.ints(cols)
    ref = w.reference_columns(w.ms, w.rs, ft)
    for j in range(w.ns.n_adv + w.ns.n_lk):
        assert ints[j] == ref[j], j
    assert w.ns.gather_public(cols.data_ptr()) == inst
    bad = w.check(ints, inst)
    assert bad and {t for t, _, _ in bad} == ({"gate"} if forge[0] == "sum" else {"copy"})
    if forge[0] in ("exp", "sum"):
        seed = b"ballot-forged"
        hinst = w.statement(honest)
        pf = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=inst)
        ph = prover_native.create_proof(w.key, w.witness().data_ptr(), prover.HashTranscript(seed), seed=9, instances=hinst)
        assert not pf.h_degree_ok and ph.h_degree_ok
        assert PV.verify_batch_native(eng, w.params, w.vk, [pf, ph], [seed, seed], instances=[inst, hinst]) == (False, [False, True])


def test_ballot_feeds_the_tally_and_decrypts_to_the_sum(eng, cref):
    """value level only: the K ciphertexts of an SB1 ballot go into pz_paillier_tally, and pz_paillier_decrypt of the product returns S"""
    from tests import decrypt_ref as DR

    bits, _, _, _, K, b = SB1
    key = DR.key(bits)
    n, g = key[0], key[1]
    Ln = _words(bits)
    rng = random.Random(0x6b40)
    ms = [3, 0, 2]
    rs = [DR.messages(n, 8, rng)[3 + i] or 1 for i in range(K)]
    c, _, _ = _k3(eng, cref, bits, n, g, ms, rs, b, want_steps=False)
    assert [cref.limbs_to_int(row) for row in c] == [P.paillier_enc_native(n, g, m, r) for m, r in zip(ms, rs)]
    prod, _ = eng.paillier_tally(Ln, cref.int_to_limbs(n, Ln), c, want_steps=False)
    sk = eng.paillier_sk(Ln, n, g, key[2], key[3])
    try:
        m_, _, fl = eng.paillier_decrypt(sk, prod.reshape(1, -1), want_r=False)
        assert fl.tolist() == [0] and cref.limbs_to_int(m_[0]) == sum(ms) == 5
    finally:
        sk.free()
