"""GPU: the mix -- the switch network's layers, the re-randomisation chains and the outputs of
pz_paillier_mix[_dev] against the independent restatement of tests/mix_ref.py in Python integers, bit for bit; every refusal; and
ballots through two mixers into decryption.  Keys: tests/golden/paillier_keys.json; every seed is fixed here."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import decrypt_ref as DR
from tests import k3_operands as KO
from tests import mix_ref as MR

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


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


def _perm(K, seed):
    p = list(range(K))
    random.Random(seed).shuffle(p)
    return p


def _inputs(bits, K, seed):
    """ciphertexts: encryptions under the fixture key, with the structured operands of tests/k3_operands.py (all-ones limbs, a lone top
    bit, 0, n^2 - 1) in their midst where K allows; r: 1, n - 1, then random"""
    rng = random.Random(seed)
    key = DR.key(bits)
    n, g = key[0], key[1]
    n2 = n * n
    ops = KO.by_name(n2, 2 * _words(bits), n)
    special = [ops["ones"], 1 << (n2.bit_length() - 2), 0, n2 - 1, ops["alt64"], ops["alt32_hi"]]
    cts = [P.paillier_enc_native(n, g, rng.randrange(n), rng.randrange(1, n)) for _ in range(K)]
    for i, v in enumerate(special[: K - 1]):
        cts[i + 1] = v
    rs = [[1, n - 1][i] if i < 2 else rng.randrange(1, n) for i in range(K)]
    return key, cts, rs


def _mix(eng, cref, bits, n, cts, sw, rs, **kw):
    Ln = _words(bits)
    lim = cref.int_to_limbs
    return eng.paillier_mix(Ln, lim(n, Ln), np.stack([lim(c, 2 * Ln) for c in cts]), np.array(list(sw), dtype=np.uint8),
                            np.stack([lim(r, Ln) for r in rs]), **kw)


def _arr(cref, values, L):
    return np.stack([cref.int_to_limbs(v, L) for v in values])


# ------------------------------------------------------------------------------------------------------------------ 1. K3
K3_SHAPES = [(128, 1), (128, 2), (128, 4), (128, 8), (264, 2), (2048, 4), (3072, 2)]


@pytest.mark.parametrize("bits,K", K3_SHAPES)
def test_k3_routes_records_and_outputs_equal_the_reference(eng, cref, bits, K):
    key, cts, rs = _inputs(bits, K, 0x3180 + bits + K)
    n = key[0]
    L = 2 * _words(bits)
    nr = MR.n_steps_r(n)
    perm = _perm(K, 0x3181 + K)
    sw = MR.route(perm)                                           # the reference's bits: the device applies what it is given
    mixed, routes, steps = _mix(eng, cref, bits, n, cts, sw, rs)
    tr = MR.mix_trace(n, cts, sw, rs)
    assert tr.routed == [cts[p] for p in perm]
    assert tr.mixed == [cts[p] * pow(r, n, n * n) % (n * n) for p, r in zip(perm, rs)]
    assert [cref.limbs_to_int(row) for row in mixed] == tr.mixed
    assert routes.shape == (len(tr.layers), K, L) and steps.shape == (K, nr + 1, 4, L)
    for l, layer in enumerate(tr.layers):
        assert np.array_equal(routes[l], _arr(cref, layer, L)), "layer %d" % l
    want = np.stack([_arr(cref, st, L) for st in MR.records(tr)])
    bad = np.nonzero((steps.reshape(-1, 4, L) != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, "record %d differs" % bad[0]
    # the values only
    m2, none_r, none_s = _mix(eng, cref, bits, n, cts, sw, rs, want_steps=False, want_routes=False)
    assert none_r is None and none_s is None and np.array_equal(m2, mixed)
    # the product's own router gives the same outputs (its bits may differ from the reference's)
    m3, _, _ = _mix(eng, cref, bits, n, cts, eng.mix_route(perm), rs, want_steps=False)
    assert np.array_equal(m3, mixed)


@pytest.mark.parametrize("which", ["identity", "reversal", "seeded"])
def test_k3_values_through_fifteen_layers(eng, cref, which):
    bits, K = 128, 256
    key, cts, rs = _inputs(bits, K, 0x3182)
    n = key[0]
    perm = {"identity": list(range(K)), "reversal": list(range(K - 1, -1, -1)), "seeded": _perm(K, 0x3183)}[which]
    assert len(MR.benes_layers(K)) == 15
    mixed, routes, none = _mix(eng, cref, bits, n, cts, eng.mix_route(perm), rs, want_steps=False)
    assert none is None and routes.shape == (15, K, 4)
    assert [cref.limbs_to_int(row) for row in routes[-1]] == [cts[p] for p in perm]
    assert [cref.limbs_to_int(row) for row in mixed] == [cts[p] * pow(r, n, n * n) % (n * n) for p, r in zip(perm, rs)]


def test_k3_one_entry_is_the_ballots_r_chain(eng, cref):
    """K = 1, no switch: the records are the r-chain and final record of pz_paillier_ballot for m = 0, b = 1 on the same r -- the last
    record's first operand excepted, which is c_1 here and g^0 = 1 there"""
    bits = 128
    key, cts, rs = _inputs(bits, 1, 0x3184)
    n, g = key[0], key[1]
    r = random.Random(0x3185).randrange(2, n)
    lim = cref.int_to_limbs
    mixed, routes, steps = _mix(eng, cref, bits, n, cts, [], [r])
    c, bsteps, nr = eng.paillier_ballot(2, lim(n, 2), lim(g, 2), np.array([0], dtype=np.uint64), lim(r, 2).reshape(1, 2), 1)
    assert routes.shape[0] == 0 and steps.shape == (1, nr + 1, 4, 4) and bsteps.shape == (1, 2 + nr + 1, 4, 4)
    assert np.array_equal(steps[0, :nr], bsteps[0, 2 : 2 + nr])
    assert np.array_equal(steps[0, nr, 1], bsteps[0, 2 + nr, 1])                                  # rn
    assert cref.limbs_to_int(bsteps[0, 2 + nr, 0]) == 1 and cref.limbs_to_int(steps[0, nr, 0]) == cts[0]
    assert cref.limbs_to_int(mixed[0]) == cts[0] * cref.limbs_to_int(c[0]) % (n * n)


def test_k3_masked_select_is_exact_on_structured_operands(eng, cref):
    """every structured operand through every switch position of K = 4 with the bit clear and set: all-ones limbs, a lone top bit,
    0, n^2 - 1 and the alternating patterns leave a switch as they entered it"""
    bits, K = 2048, 4
    n = DR.key(bits)[0]
    n2 = n * n
    L = 2 * _words(bits)
    ops = KO.operands(n2, L, n)
    vals = [ops["ones"], 1 << (n2.bit_length() - 2), 0, n2 - 1, ops["alt64"], ops["alt32_hi"], ops["alt32_lo"], 1]
    for at, sw in enumerate([[0] * 6, [1] * 6, [1, 0, 0, 1, 1, 0]]):
        cts = vals[at: at + 4] if at < 2 else [vals[4], vals[0], vals[7], vals[3]]
        mixed, routes, _ = _mix(eng, cref, bits, n, cts, sw, [1] * K, want_steps=False)
        tr = MR.mix_trace(n, cts, sw, [1] * K)
        for l, layer in enumerate(tr.layers):
            assert np.array_equal(routes[l], _arr(cref, layer, L)), (at, l)
        assert [cref.limbs_to_int(row) for row in mixed] == tr.routed                              # r = 1: the product is d_i itself


def test_k3_refusals_in_order_with_untouched_outputs(eng, cref):
    from paillier_halo2_amd import _lib

    bits, K = 128, 4
    key, cts, rs = _inputs(bits, K, 0x3186)
    n = key[0]
    cts = [c % (n * n) for c in cts]
    lim = cref.int_to_limbs
    nr = MR.n_steps_r(n)
    need = K * (nr + 1)
    n_, c_, r_ = lim(n, 2), _arr(cref, cts, 4), _arr(cref, rs, 2)
    sw = np.array(MR.route(_perm(K, 0x3187)), dtype=np.uint8)
    zero_n = lim(0, 2)
    routes = np.full((3, K, 4), 0xA5, dtype=np.uint64)
    steps = np.full((need, 4, 4), 0xA5, dtype=np.uint64)
    out = np.full((K, 4), 0xA5, dtype=np.uint64)

    def call(limbs=2, count=K, nn=n_, cc=c_, bb=sw, rr=r_, cap=need, oo=out):
        p = lambda a: None if a is None else a.ctypes.data
        return eng.L.pz_paillier_mix(eng.ctx, limbs, count, p(nn), p(cc), p(bb), p(rr), p(routes), p(steps), cap, p(oo))

    bad_bit = sw.copy()
    bad_bit[-1] = 2
    INV, UNS, CAP, MSG, ZERO = (_lib.PZ_ERR_INVALID, _lib.PZ_ERR_UNSUPPORTED, _lib.PZ_ERR_CAPACITY, _lib.PZ_ERR_MESSAGE_RANGE,
                                _lib.PZ_ERR_ZERO_MODULUS)
    # each refusal alone
    for kw in (dict(nn=None), dict(cc=None), dict(bb=None), dict(rr=None), dict(oo=None), dict(limbs=0), dict(count=0), dict(count=3),
               dict(count=6), dict(count=2048)):
        assert call(**kw) == INV, kw
    assert call(limbs=65) == UNS
    assert call(cap=need - 1) == CAP
    assert call(bb=bad_bit) == MSG
    assert call(nn=zero_n) == ZERO
    # the order: each one wins over all that follow it
    assert call(count=3, limbs=65, cap=0, bb=bad_bit, nn=zero_n) == INV
    assert call(limbs=65, cap=0, bb=bad_bit, nn=zero_n) == UNS
    assert call(cap=0, bb=bad_bit, nn=zero_n) == CAP
    assert call(bb=bad_bit, nn=zero_n) == MSG
    # a ciphertext of exactly n^2 is found by the kernel
    over = _arr(cref, [cts[0], n * n, cts[2], cts[3]], 4)
    assert call(cc=over) == _lib.PZ_ERR_RANGE
    assert (routes == 0xA5).all() and (steps == 0xA5).all() and (out == 0xA5).all()
    # the context serves an honest call afterwards
    assert call() == 0
    tr = MR.mix_trace(n, cts, sw.tolist(), rs)
    assert [cref.limbs_to_int(row) for row in out] == tr.mixed
    assert np.array_equal(routes, np.stack([_arr(cref, layer, 4) for layer in tr.layers]))
    assert tuple(cref.limbs_to_int(steps[-1, f]) for f in range(4)) == MR.records(tr)[-1]
    # the Python layer reports the status
    assert _status(lambda: _mix(eng, cref, bits, n, cts, bad_bit, rs)) == MSG


@pytest.mark.parametrize("bits,K", [(128, 1), (128, 8), (264, 2)])
def test_k3_dev_form_equals_the_host_form(eng, cref, bits, K):
    import torch

    key, cts, rs = _inputs(bits, K, 0x3188 + K)
    n = key[0]
    Ln = _words(bits)
    L = 2 * Ln
    lim = cref.int_to_limbs
    sw = eng.mix_route(_perm(K, 0x3189))
    mixed, routes, steps = _mix(eng, cref, bits, n, cts, sw, rs)
    layers, per = routes.shape[0], steps.shape[1]
    d_routes = torch.zeros((max(layers, 1), K, L), dtype=torch.int64, device="cuda")
    d_steps = torch.zeros((K, per, 4, L), dtype=torch.int64, device="cuda")
    args = (Ln, lim(n, Ln), _arr(cref, cts, L), sw, _arr(cref, rs, Ln))
    got = eng.paillier_mix_dev(*args, d_routes.data_ptr(), d_steps.data_ptr(), K * per)
    assert np.array_equal(got, mixed)
    assert np.array_equal(d_routes.cpu().numpy().view(np.uint64)[:layers], routes)
    assert np.array_equal(d_steps.cpu().numpy().view(np.uint64), steps)
    assert np.array_equal(eng.paillier_mix_dev(*args, 0, 0, 0), mixed)                          # neither buffer: the values only
    from paillier_halo2_amd import _lib

    assert _status(lambda: eng.paillier_mix_dev(*args, d_routes.data_ptr(), d_steps.data_ptr(), K * per - 1)) == _lib.PZ_ERR_CAPACITY


# ------------------------------------------------------------------------------------------------------------------ 2. end to end
def test_ballots_through_two_mixers_decrypt_in_the_predicted_order(eng, cref):
    """K = 4 ballots of distinct small values from pz_paillier_ballot go through two mixers with different permutations; decryption
    of the second mixer's outputs gives the values in the order perm_2 o perm_1 predicts, and no output is an input ciphertext"""
    bits, K = 128, 4
    key = DR.key(bits)
    n, g = key[0], key[1]
    Ln = _words(bits)
    lim = cref.int_to_limbs
    rng = random.Random(0x318A)
    ms = [5, 9, 2, 14]
    r0 = [rng.randrange(1, n) for _ in range(K)]
    c0, _, _ = eng.paillier_ballot(Ln, lim(n, Ln), lim(g, Ln), np.array(ms, dtype=np.uint64), _arr(cref, r0, Ln), 4, want_steps=False)
    cts0 = [cref.limbs_to_int(row) for row in c0]
    assert cts0 == [P.paillier_enc_native(n, g, m, r) for m, r in zip(ms, r0)]
    perm1, perm2 = [2, 0, 3, 1], [3, 2, 0, 1]
    r1, r2 = ([rng.randrange(1, n) for _ in range(K)] for _ in range(2))
    m1, _, _ = eng.paillier_mix(Ln, lim(n, Ln), c0, eng.mix_route(perm1), _arr(cref, r1, Ln), want_steps=False, want_routes=False)
    m2, _, _ = eng.paillier_mix(Ln, lim(n, Ln), m1, eng.mix_route(perm2), _arr(cref, r2, Ln), want_steps=False, want_routes=False)
    cts1, cts2 = ([cref.limbs_to_int(row) for row in m] for m in (m1, m2))
    assert not set(cts0) & set(cts1) and not set(cts0) & set(cts2) and not set(cts1) & set(cts2)
    sk = eng.paillier_sk(Ln, n, g, key[2], key[3])
    try:
        got, _, fl = eng.paillier_decrypt(sk, m2, want_r=False)
        assert fl.tolist() == [0] * K
        both = [perm1[perm2[i]] for i in range(K)]                    # output i of mixer 2 holds mixer 1's output perm2[i]
        assert [cref.limbs_to_int(row) for row in got] == [ms[j] for j in both] == [9, 14, 2, 5]
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------------------------ 3. K4
from tests import public_ref as PR  # noqa: E402

R = P.FR_R
BF = 6
SM4 = (128, 64, 13, 14, 4)         # the ballot's main shape with K = 4: three layers, break points crossed inside the chains
SM2 = (264, 88, 11, 14, 2)         # the reference's add-test key size on 88-bit limbs: K3's fields are 10 words, K4's 9
SM1 = (128, 64, 10, 13, 1)         # one ciphertext: no switch, a proven re-randomisation
SM2S = (128, 64, 10, 13, 2)        # one switch


def _mix_inputs(bits, K, seed):
    rng = random.Random(seed)
    key = DR.key(bits)
    n, g = key[0], key[1]
    cts = [P.paillier_enc_native(n, g, rng.randrange(n), rng.randrange(1, n)) for _ in range(K)]
    rs = [[1, n - 1][i] if i < 2 else rng.randrange(1, n) for i in range(K)]
    return n, cts, rs, _perm(K, seed + 1)


def _ref_trace(n, cts, rs, sw, bits, W, forge=None):
    return MR.mix_trace(n, cts, sw, rs, forge=forge, limb_bits=W, limbs=2 * (bits // W))


def _k3_dev(eng, cref, bits, n, cts, sw, rs):
    """pz_paillier_mix_dev's routes and records left on the device as they are -> (mixed integers, d_routes, d_steps)"""
    import torch

    wn = _words(bits)
    K = len(cts)
    per = MR.n_steps_r(n) + 1
    layers = len(MR.benes_layers(K))
    d_routes = torch.zeros((max(layers, 1), K, 2 * wn), dtype=torch.int64, device="cuda")
    d_steps = torch.zeros((K, per, 4, 2 * wn), dtype=torch.int64, device="cuda")
    lim = cref.int_to_limbs
    mixed = eng.paillier_mix_dev(wn, lim(n, wn), _arr(cref, cts, 2 * wn), np.array(list(sw), dtype=np.uint8), _arr(cref, rs, wn),
                                 d_routes.data_ptr(), d_steps.data_ptr(), K * per)
    return [cref.limbs_to_int(row) for row in mixed], d_routes, d_steps


def _mix_k4_inputs(cref, bits, n, cts, rs, res):
    lim = cref.int_to_limbs
    wn, wl = _words(bits), _words(2 * bits)
    return np.concatenate([lim(n, wn)] + [lim(c, wl) for c in cts] + [lim(r, wn) for r in rs] + [lim(v, wl) for v in res])


@pytest.mark.parametrize("shape", [SM1, SM2S, SM4, SM2], ids=["K1", "K2", "K4", "264-88"])
def test_k4_dense_stream_and_break_point_columns_equal_the_reference(eng, cref, shape):
    import torch
    from paillier_halo2_amd import _lib, layout

    bits, W, lb, k, K = shape
    Ln, n_rows = bits // W, 1 << k
    n, cts, rs, perm = _mix_inputs(bits, K, 0x31E0 + K)
    sw = MR.route(perm)
    tr = _ref_trace(n, cts, rs, sw, bits, W)
    nr = MR.n_steps_r(n)
    want_a, want_l, seg = MR.mix_cells(n, cts, rs, tr.mixed, bits, W, lb, tr)
    assert seg["satisfied"]
    na, nl = eng.mix_cells(Ln, W, lb, K, nr)
    assert (na, nl) == (len(want_a), len(want_l))
    pub = eng.mix_public_cells(Ln, W, lb, K, nr).tolist()
    assert len(pub) == Ln + 2 * K * 2 * Ln
    assert [want_a[c] for c in pub] == MR.statement(n, cts, tr.mixed, bits, W)
    mixed, d_routes, d_steps = _k3_dev(eng, cref, bits, n, cts, sw, rs)
    assert mixed == tr.mixed
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    inputs = _mix_k4_inputs(cref, bits, n, cts, rs, tr.mixed)
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.mix_expand_dev(Ln, W, lb, K, nr, inputs, sw, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d (network at %d, outputs at %d)" % (len(bad), bad[0], seg["network"][0], seg["outputs"][0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    # ---- the same stream in break-point columns
    rb = layout.row_budget(k)
    starts = layout.break_points(MR.mix_gate_mask(K, bits, W, lb, nr), rb.max_rows)
    A_used = starts.shape[0] - 1
    A, Lk = rb.columns_for(na, filled=A_used), rb.columns_for(nl)
    full = np.concatenate([starts, np.full(A - A_used, na, dtype=np.uint64)])
    d_starts = torch.from_numpy(full.astype(np.int64)).cuda()
    cols = torch.zeros((A + Lk + 1, n_rows, 4), dtype=torch.int64, device="cuda")
    eng.mix_expand_cols_dev(Ln, W, lb, K, nr, inputs, sw, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(),
                            cols[A].data_ptr(), d_starts.data_ptr(), A, rb.max_rows, rb.max_rows, n_rows)
    eng.sync()
    want_cols = MR.place(want_a, want_l, full, A, Lk, rb.max_rows, k, [])
    host = cols.cpu().numpy().view(np.uint64)
    for j in range(A + Lk + 1):
        assert cref.fr_mont_to_ints(host[j]) == want_cols[j], j
    assert A_used >= 2
    if K > 1:       # a switch byte above 1 is refused by both forms
        over = list(sw)
        over[0] = 2
        assert _status(lambda: eng.mix_expand_dev(Ln, W, lb, K, nr, inputs, over, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(),
                                                  d_adv.data_ptr(), d_lk.data_ptr())) == _lib.PZ_ERR_MESSAGE_RANGE
    # the by-kind entry points keep refusing kind 8; a count that is no power of two has no stream
    assert _status(lambda: eng.circuit_cells(8, Ln, W, lb, 0, nr)) == _lib.PZ_ERR_INVALID
    assert _status(lambda: eng.mix_cells(Ln, W, lb, 3, nr)) == _lib.PZ_ERR_INVALID
    assert _status(lambda: eng.mix_cells(Ln, W, lb, K, 0)) == _lib.PZ_ERR_INVALID


def test_k4_dense_stream_of_a_mismatching_result_equals_the_reference(eng, cref):
    """output 1's claimed ciphertext differs from the computed one in a middle limb only, output 0's matches: the running-equality chain
    of output 1 drops there and stays down, the is_zero inverse cell of that limb is a true inverse -- the cells the matching streams
    above never reach"""
    import torch

    bits, W, lb, k, K = SM2S
    Ln = bits // W
    n, cts, rs, perm = _mix_inputs(bits, K, 0x31EA)
    sw = MR.route(perm)
    tr = _ref_trace(n, cts, rs, sw, bits, W)
    nr = MR.n_steps_r(n)
    res = [tr.mixed[0], tr.mixed[1] ^ (1 << (W + 5))]   # limb 1 of 4
    want_a, want_l, seg = MR.mix_cells(n, cts, rs, res, bits, W, lb, tr)
    assert not seg["satisfied"]
    na, nl = eng.mix_cells(Ln, W, lb, K, nr)
    assert (na, nl) == (len(want_a), len(want_l))
    mixed, d_routes, d_steps = _k3_dev(eng, cref, bits, n, cts, sw, rs)
    assert mixed == tr.mixed
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.mix_expand_dev(Ln, W, lb, K, nr, _mix_k4_inputs(cref, bits, n, cts, rs, res), sw, d_routes.data_ptr(), d_steps.data_ptr(),
                       d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d (outputs at %d)" % (len(bad), bad[0], seg["outputs"][0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l


# ------------------------------------------------------------------------------------------------------------------ 4. structure
@pytest.mark.parametrize("shape", [SM4, SM1], ids=["K4", "K1"])
@pytest.mark.parametrize("expose", [False, True])
def test_native_structure_equals_the_python_generator(eng, shape, expose):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout, prover_native

    bits, W, lb, k, K = shape
    n = DR.key(bits)[0]
    nr = MR.n_steps_r(n)
    sa = CS.stream_structure("mix", bits, W, lb, exp_r=n, count=K)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=expose)
    ns = prover_native.NativeStructure(eng, "mix", bits, W, lb, k, exp_r=n, count=K, expose=expose)
    try:
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], 0, nr)
        assert ns.starts().tolist() == starts.tolist()
        assert ns.starts()[: ns.n_adv_used + 1].tolist() == layout.break_points(MR.mix_gate_mask(K, bits, W, lb, nr), ns.max_rows).tolist()
        assert ns.constants() == [int(c) for c in cs.constants]
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        Ln = bits // W
        assert (ns.n_instance, ns.n_public) == ((1, Ln + 2 * K * 2 * Ln) if expose else (0, 0))
        if expose:
            assert ns.public_cells() == cs.public_cells
    finally:
        ns.free()
    for count in (0, 3, 6, 2048):
        with pytest.raises(Exception):
            prover_native.NativeStructure(eng, "mix", bits, W, lb, k, exp_r=n, count=count)


# ------------------------------------------------------------------------------------------------------------------ 5. / 6. the proof
class World:
    """SRS with a known toxic scalar, both structures with the instance column, both keys, witnesses from K3 -> K4"""

    def __init__(self, eng, cref, shape, seed):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.bits, self.W, self.lb, self.k, self.K = shape
        bits, W, lb, k, K = shape
        self.n_rows = n = 1 << k
        self.nn, self.cts, self.rs, self.perm = _mix_inputs(bits, K, seed)
        self.nr = MR.n_steps_r(self.nn)
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
        self.ns = prover_native.NativeStructure(eng, "mix", bits, W, lb, k, exp_r=self.nn, count=K, expose=True)
        self.sa = CS.stream_structure("mix", bits, W, lb, exp_r=self.nn, count=K)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)
        self.structure = self.ns.download()

    def trace(self, perm=None, rs=None, forge=None, cts=None, sw=None):
        sw = MR.route(self.perm if perm is None else perm) if sw is None else sw
        return _ref_trace(self.nn, self.cts if cts is None else cts, self.rs if rs is None else rs, sw, self.bits, self.W, forge=forge)

    def statement(self, trace, cts=None):
        return MR.statement(self.nn, self.cts if cts is None else cts, trace.mixed, self.bits, self.W)

    def witness(self, perm=None, rs=None):
        """K4's columns [m'][2^k][4] from K3's routes and records, both left on the device"""
        import torch

        eng, cref, ns = self.eng, self.cref, self.ns
        rs = self.rs if rs is None else rs
        sw = eng.mix_route(self.perm if perm is None else perm)      # the product's own router
        mixed, d_routes, d_steps = _k3_dev(eng, cref, self.bits, self.nn, self.cts, sw, rs)
        d_mod = torch.from_numpy(cref.int_to_limbs(self.nn ** 2, _words(2 * self.bits)).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        eng.mix_expand_cols_dev(self.bits // self.W, self.W, self.lb, self.K, self.nr, _mix_k4_inputs(cref, self.bits, self.nn, self.cts, rs, mixed),
                                sw, d_routes.data_ptr(), d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(),
                                ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, self.n_rows)
        eng.sync()
        return cols

    def reference_columns(self, trace, cts=None, rs=None):
        cts = self.cts if cts is None else cts
        want_a, want_l, _ = MR.mix_cells(self.nn, cts, self.rs if rs is None else rs, trace.mixed, self.bits, self.W, self.lb, trace)
        return MR.place(want_a, want_l, self.ns.starts(), self.ns.n_adv, self.ns.n_lk, self.ns.max_rows, self.k, [])

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
        """tally_ref.check_columns on a witness under the NATIVE structure"""
        ns = self.ns
        sel, mc, mr = self.structure
        ck = ns.n_adv + ns.n_lk
        ints = list(ints)
        ints[ck] = [c % R for c in ns.constants()] + ints[ck][ns.n_constants:]
        ints[ck + 1] = list(instances) + ints[ck + 1][len(instances):]
        return MR.check_columns(sel, mc, mr, range(1 << self.lb), ints, ns.n_lk)

    def close(self):
        self.key.free()
        self.ns.free()
        self.bl.free()
        self.bm.free()


@pytest.fixture(scope="module")
def world(eng, cref):
    w = World(eng, cref, SM4, 0x31F0)
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
    assert inst == w.statement(tr) and len(inst) == 2 + 2 * 4 * 4
    ints = w.ints(cols)
    ref = w.reference_columns(w.trace(sw=eng.mix_route(w.perm).tolist()))        # (the witness was routed by the product)
    for j in range(w.ns.n_adv + w.ns.n_lk):
        assert ints[j] == ref[j], j
    assert w.check(ints, inst) == []
    assert w.ns.n_adv_used >= 40                            # break points are crossed inside every chain
    # the two keys describe one circuit
    a, b = w.key.vk_commitments(), w.pk.vk_commitments()
    assert np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])


def test_connected_proof_both_provers_two_permutations_one_key(eng, cref, world):
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    tr_a = w.trace()
    perm_b, rs_b = [w.perm[1], w.perm[0], w.perm[3], w.perm[2]], [w.rs[2], 7, w.rs[3], w.rs[1]]
    tr_b = w.trace(perm_b, rs_b)
    good, other = w.statement(tr_a), w.statement(tr_b)
    kw = dict(enc_bits=w.bits, limb_bits=w.W)
    assert PV.public_inputs("mix", n=w.nn, cts=w.cts, mixed=tr_a.mixed, **kw) == good
    assert PV.public_inputs("mix", n=w.nn, cts=w.cts, mixed=tr_b.mixed, **kw) == other != good
    seeds = [b"mix-stepper", b"mix-python", b"mix-second"]
    cols = w.witness()
    p0 = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seeds[0]), seed=5, instances=good)
    p1 = prover.create_proof(w.pk, w.witness(), prover.HashTranscript(seeds[1]), seed=6, tile=8, instances=good)
    cols2 = w.witness(perm_b, rs_b)
    assert w.ns.gather_public(cols2.data_ptr()) == other
    p2 = prover_native.create_proof(w.key, cols2.data_ptr(), prover.HashTranscript(seeds[2]), seed=7, instances=other)       # the SAME key
    proofs, inst = [p0, p1, p2], [good, good, other]
    for pr, seed, st in zip(proofs, seeds, inst):
        assert _oracle_checks(cref, w, pr, seed, st) == (True, True, True)
    assert PV.verify_batch(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])
    # permutation A's proofs under permutation B's statement
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[other, other, other]) == (False, [False, False, True])
    # ... and against `mixed` with two entries exchanged: the proof names which output stands where
    swapped = PV.public_inputs("mix", n=w.nn, cts=w.cts, mixed=[tr_a.mixed[1], tr_a.mixed[0]] + tr_a.mixed[2:], **kw)
    assert PV.verify_batch(eng, w.params, w.vk, proofs, seeds, instances=[swapped, swapped, other]) == (False, [False, False, True])
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[swapped, swapped, other]) == (False, [False, False, True])


def test_one_proven_rerandomisation(eng, cref):
    """K = 1: c' holds what c holds"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = World(eng, cref, SM1, 0x3200)
    try:
        tr = w.trace(rs=[w.nn - 2])
        assert tr.mixed == [w.cts[0] * pow(w.nn - 2, w.nn, w.nn ** 2) % w.nn ** 2] and tr.layers == []
        cols = w.witness(rs=[w.nn - 2])
        inst = PV.public_inputs("mix", n=w.nn, cts=w.cts, mixed=tr.mixed, enc_bits=w.bits, limb_bits=w.W)
        assert w.ns.gather_public(cols.data_ptr()) == inst == w.statement(tr)
        assert w.check(w.ints(cols), inst) == []
        seed = b"mix-one"
        pr = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=3, instances=inst)
        assert PV.verify_batch(eng, w.params, w.vk, [pr], [seed], instances=[inst]) == (True, [True])
        other = PV.public_inputs("mix", n=w.nn, cts=w.cts, mixed=[tr.mixed[0] ^ 1], enc_bits=w.bits, limb_bits=w.W)
        assert PV.verify_batch(eng, w.params, w.vk, [pr], [seed], instances=[other]) == (False, [False])
    finally:
        w.close()


FORGES = [("bit", 1, 0, 2), ("dup", 0, 1), ("src", 1, 2, 1), ("in", 3, 1), ("rn", 2, 1), ("d", 3, 1)]      # (not output 1: its r = n - 1 has
                                                                                                              # r^n = n^2 - 1, and rn + 1 = n^2 leaves the output 0)


@pytest.mark.parametrize("forge", FORGES, ids=lambda f: f[0])
def test_forged_edges_are_rejected(eng, cref, world, forge):
    """a switch bit of 2; a switch whose selects run under different bits (one input twice, one dropped); a select reading the previous
    layer's limb + 1; layer 0 reading c_4 + 1 under the exposed c_4; the final block fed rn + 1, or d + 1 -- each with everything
    downstream, the claimed outputs and the statement recomputed consistently, placed in the NATIVE structure's columns.  Every lookup
    and every final equality holds; a copy constraint objects (the bit of 2: assert_bit's gate).  For the bit and the dup a proof made
    from the forged witness is refused by verification."""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    cts, sw = w.cts, None
    if forge[0] == "bit":       # equal inputs at the forged switch: the bit of 2 changes no value, assert_bit's gate ALONE objects
        cts, sw = [w.cts[0], w.cts[1], w.cts[0], w.cts[3]], [0] * 6
    ft = w.trace(forge=forge, cts=cts, sw=sw)
    honest = w.trace(cts=cts, sw=sw)
    assert (ft.mixed != honest.mixed) == (forge[0] != "bit")
    inst = w.statement(ft, cts)
    assert inst == PV.public_inputs("mix", n=w.nn, cts=cts, mixed=ft.mixed, enc_bits=w.bits, limb_bits=w.W)      # a statement a verifier accepts
    ref = w.reference_columns(ft, cts)
    bad = w.check(ref + [[0] * w.n_rows], inst)
    assert bad and {t for t, _, _ in bad} == ({"gate"} if forge[0] == "bit" else {"copy"})
    if forge[0] in ("bit", "dup"):
        seed = b"mix-forged"
        cols = w.upload(ref)
        assert w.ns.gather_public(cols.data_ptr()) == inst
        hcols = w.upload(w.reference_columns(honest, cts))
        hinst = w.statement(honest, cts)
        pf = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=inst)
        ph = prover_native.create_proof(w.key, hcols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=hinst)
        assert not pf.h_degree_ok and ph.h_degree_ok
        assert PV.verify_batch(eng, w.params, w.vk, [pf, ph], [seed, seed], instances=[inst, hinst]) == (False, [False, True])


# ------------------------------------------------------------------------------------------------------------------ 7. K3 under structured n
# n of 8, 9, 31, 32, 33 and 49 limbs that are runs of ones and zeros, and two Mersenne-product keys, as
# section 15.13 runs wtally, ballot, encrypt and partial: k_mix_rerand's r^n chain runs over every bit of such an n
STRUCT_SHAPES = [(ln, tb) for ln in (8, 9, 31, 32, 33, 49) for tb in (1, 64)] + [("mersenne", 3), ("mersenne", 5)]


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
    """K = 1 and K = 2 (the switch set, and clear at a one-bit top limb): c in {1, n + 1, n^2 - 1, an encryption} and r in {1, n - 1, 2^k}, every record; a
    ciphertext of exactly n^2 is refused with PZ_ERR_RANGE and nothing is written"""
    from paillier_halo2_amd import _lib

    Ln, cases = _struct_ns(ln, tb)
    L = 2 * Ln
    for cls, n in cases:
        n2 = n * n
        enc = (1 + KO.by_name(n, Ln)["alt64"] * n) * pow(3, n, n2) % n2
        two_k = 1 << (n.bit_length() - 2)
        runs = [([1], [], [n - 1]), ([n2 - 1], [], [two_k]), ([n + 1, enc], [1 if tb != 1 else 0], [1, two_k])]
        for cts, sw, rs in runs:
            K = len(cts)
            where = (ln, tb, cls, K, sw)
            mixed, routes, steps = eng.paillier_mix(Ln, _bytes_rows([n], Ln)[0], _bytes_rows(cts, L), np.array(sw, dtype=np.uint8), _bytes_rows(rs, Ln))
            tr = MR.mix_trace(n, cts, sw, rs)
            perm = list(range(K)) if not sw or sw[0] == 0 else [1, 0]
            assert tr.mixed == [cts[p] * pow(r, n, n2) % n2 for p, r in zip(perm, rs)], where
            assert [int.from_bytes(row.tobytes(), "little") for row in mixed] == tr.mixed, where
            for l, layer in enumerate(tr.layers):
                assert np.array_equal(routes[l], _bytes_rows(layer, L)), where + ("layer %d" % l,)
            want = MR.records(tr)
            want_arr = _bytes_rows([v for st in want for v in st], L).reshape(len(want), 4, L)
            assert steps.shape == (K, MR.n_steps_r(n) + 1, 4, L), where
            bad = np.nonzero((steps.reshape(-1, 4, L) != want_arr).any(axis=(1, 2)))[0]
            assert bad.size == 0, where + ("record %d differs" % bad[0],)
        # a ciphertext of exactly n^2: the kernel's range bit, outputs untouched
        K, nr = 2, MR.n_steps_r(n)
        routes = np.full((1, K, L), 0xA5, dtype=np.uint64)
        steps = np.full((K * (nr + 1), 4, L), 0xA5, dtype=np.uint64)
        out = np.full((K, L), 0xA5, dtype=np.uint64)
        n_, c_, r_, b_ = _bytes_rows([n], Ln), _bytes_rows([n + 1, n2], L), _bytes_rows([1, 2], Ln), np.array([1], dtype=np.uint8)
        rc = eng.L.pz_paillier_mix(eng.ctx, Ln, K, n_.ctypes.data, c_.ctypes.data, b_.ctypes.data, r_.ctypes.data, routes.ctypes.data,
                                   steps.ctypes.data, K * (nr + 1), out.ctypes.data)
        assert rc == _lib.PZ_ERR_RANGE and (routes == 0xA5).all() and (steps == 0xA5).all() and (out == 0xA5).all(), (ln, tb, cls)
