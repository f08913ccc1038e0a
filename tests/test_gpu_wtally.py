"""GPU: the weighted tally circuit (kind 4 / "wtally") through every layer -- the chains and the product tree
(K3), the cell stream (K4), the native structure generator, and ONE connected proof with the statement "C is the product of exactly
these c_i raised to exactly these w_i under n" by both provers -- against the independent restatement of tests/wtally_ref.py in
Python integers.  Every comparison is exact.

Main shape S1w: 128-bit n, 64-bit limbs, lookup_bits 10, k = 11, B = 3, W = 3 -- an odd B (the carried power), break points crossed
many times, 21 public values."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import public_ref as PR
from tests import wtally_ref as WR

pytestmark = pytest.mark.gpu

R = P.FR_R
BF = 6
S1W = (128, 64, 10, 11, 3, 3)
S2W = (264, 88, 11, 12, 2, 2)       # the reference's add-test key size on 88-bit limbs


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _weights(B, wb, rng):
    """0, 2^W - 1 and a lone top bit where B allows, random below 2^W otherwise"""
    special = [0, (1 << wb) - 1, 1 << (wb - 1)]
    return [special[i] if i < 3 else rng.randrange(1 << wb) for i in range(B)]


def _inputs(bits, B, wb, seed):
    rng = random.Random(seed)
    n = P.synth_paillier_inputs(bits, seed)[0]
    return n, [rng.randrange(1, n * n - 1) for _ in range(B)], _weights(B, wb, rng)


def _words(bits):
    return -(-bits // 64)


def _u64(ws):
    return np.array([int(w) for w in ws], dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------ 1. K3
K3_SHAPES = [(128, 1, 1), (128, 1, 64), (128, 3, 3), (128, 5, 8), (128, 300, 2), (264, 3, 5), (2048, 3, 4), (3072, 2, 2)]


@pytest.mark.parametrize("bits,B,wb", K3_SHAPES)
def test_k3_records_equal_the_reference(eng, cref, bits, B, wb):
    n, cts, weights = _inputs(bits, B, wb, 0x3a20 + 64 * B + wb)
    vectors = [weights]
    if B == 1:      # one chain carries one weight: zero, all ones and the lone top bit each get a run
        vectors = [[0], [(1 << wb) - 1], [1 << (wb - 1)]]
    Ln = _words(bits)
    L = 2 * Ln
    lim = cref.int_to_limbs
    n_w, cts_w = lim(n, Ln), np.stack([lim(v, L) for v in cts])
    for ws in vectors:
        c, steps = eng.paillier_wtally(Ln, n_w, cts_w, _u64(ws), wb)
        root, chains, tree, powers, _ = WR.wtally_trace(n, cts, ws, wb)
        want = WR.records(chains, tree)
        assert steps.shape == (2 * B * wb + B - 1, 4, L) == (len(want), 4, L) and cref.limbs_to_int(c) == root
        for t, st in enumerate(want):
            assert tuple(cref.limbs_to_int(steps[t, f]) for f in range(4)) == st, t
        c2, none = eng.paillier_wtally(Ln, n_w, cts_w, _u64(ws), wb, want_steps=False)
        assert none is None and np.array_equal(c2, c)
        if B == 1:
            assert root == pow(cts[0], ws[0], n * n)


def test_k3_refusals(eng, cref):
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import _lib

    B, wb = 3, 3
    n, cts, weights = _inputs(128, B, wb, 0x3a21)
    lim = cref.int_to_limbs
    arr = lambda vs: np.stack([lim(v, 4) for v in vs])

    def status(fn):
        with pytest.raises(pz.PzError) as e:
            fn()
        return e.value.status

    for bad in range(B):          # a ciphertext EQUAL to n^2, in every position (the last is the carried power)
        vs = list(cts)
        vs[bad] = n * n
        assert status(lambda: eng.paillier_wtally(2, lim(n, 2), arr(vs), _u64([1, 1, 1]), wb)) == _lib.PZ_ERR_RANGE
    assert status(lambda: eng.paillier_wtally(2, lim(0, 2), arr(cts), _u64(weights), wb)) == _lib.PZ_ERR_ZERO_MODULUS
    assert status(lambda: eng.paillier_wtally(2, lim(n, 2), arr(cts), _u64([0, 8, 1]), wb)) == _lib.PZ_ERR_MESSAGE_RANGE     # 8 = 2^W
    assert status(lambda: eng.paillier_wtally(2, lim(n, 2), arr(cts), _u64(weights), 0)) == _lib.PZ_ERR_INVALID
    assert status(lambda: eng.paillier_wtally(2, lim(n, 2), arr(cts), _u64(weights), 65)) == _lib.PZ_ERR_INVALID
    out = np.zeros(4, dtype=np.uint64)
    a, w_, n_ = arr(cts), _u64(weights), lim(n, 2)
    need = 2 * B * wb + B - 1
    steps = np.zeros((need, 4, 4), dtype=np.uint64)
    call = lambda count, cap: eng.L.pz_paillier_wtally(eng.ctx, 2, count, wb, n_.ctypes.data, a.ctypes.data, w_.ctypes.data, steps.ctypes.data, cap,
                                                       out.ctypes.data)
    assert call(0, need) == _lib.PZ_ERR_INVALID
    assert call(65537, need) == _lib.PZ_ERR_INVALID
    assert call(B, need - 1) == _lib.PZ_ERR_CAPACITY
    # the context still serves an honest call
    c, _ = eng.paillier_wtally(2, n_, a, w_, wb)
    assert cref.limbs_to_int(c) == WR.wtally_trace(n, cts, weights, wb)[0]


# ------------------------------------------------------------------------------------------------------------------ 2. K4
def _device_records(eng, cref, bits, n, cts, weights, wb, trace=None):
    """the 2 B W + B - 1 records on the device, fields of ceil(2 bits / 64) words: K3's own (trace = None), or a given trace's (the
    forged ones)"""
    import torch

    Ln, L64 = _words(bits), _words(2 * bits)
    lim = cref.int_to_limbs
    if trace is None:
        c, rec = eng.paillier_wtally(Ln, lim(n, Ln), np.stack([lim(v, 2 * Ln) for v in cts]), _u64(weights), wb)
        assert cref.limbs_to_int(c) == WR.wtally_trace(n, cts, weights, wb)[0] and not rec[:, :, L64:].any()
        rec = np.ascontiguousarray(rec[:, :, :L64])
    else:
        rec = np.stack([np.stack([lim(v, L64) for v in st]) for st in WR.records(trace[1], trace[2])])
    return torch.from_numpy(rec.astype(np.int64)).cuda()


def _wtally_inputs(cref, bits, n, cts, weights, res):
    lim = cref.int_to_limbs
    return np.concatenate([lim(n, _words(bits))] + [lim(v, _words(2 * bits)) for v in cts] + [_u64(weights), lim(res, _words(2 * bits))])


@pytest.mark.parametrize("shape", [S1W, S2W])
def test_k4_dense_stream_and_break_point_columns_equal_the_reference(eng, cref, shape):
    import torch
    from paillier_halo2_amd import layout

    bits, W, lb, k, B, wb = shape
    Ln, n_rows = bits // W, 1 << k
    n, cts, weights = _inputs(bits, B, wb, 0x3a22)
    root = WR.wtally_trace(n, cts, weights, wb)[0]
    want_a, want_l, _ = WR.wtally_cells(n, cts, weights, root, wb, bits, W, lb)
    ng, nr = 2 * B * wb, B - 1
    na, nl = eng.circuit_cells(4, Ln, W, lb, ng, nr)
    assert (na, nl) == (len(want_a), len(want_l))
    d_steps = _device_records(eng, cref, bits, n, cts, weights, wb)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    inputs = _wtally_inputs(cref, bits, n, cts, weights, root)
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.circuit_expand_dev(4, Ln, W, lb, inputs, d_steps.data_ptr(), ng, nr, d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    # ---- the same stream in break-point columns
    rb = layout.row_budget(k)
    starts = layout.break_points(WR.wtally_gate_mask(B, wb, bits, W, lb), rb.max_rows)
    A_used = starts.shape[0] - 1
    A, Lk = rb.columns_for(na, filled=A_used), rb.columns_for(nl)
    full = np.concatenate([starts, np.full(A - A_used, na, dtype=np.uint64)])
    d_starts = torch.from_numpy(full.astype(np.int64)).cuda()
    cols = torch.zeros((A + Lk + 1, n_rows, 4), dtype=torch.int64, device="cuda")
    eng.circuit_expand_cols_dev(4, Ln, W, lb, inputs, d_steps.data_ptr(), ng, nr, d_mod.data_ptr(), cols.data_ptr(), cols[A].data_ptr(),
                                d_starts.data_ptr(), A, rb.max_rows, rb.max_rows, n_rows)
    eng.sync()
    want_cols = WR.place(want_a, want_l, full, A, Lk, rb.max_rows, k, [])
    host = cols.cpu().numpy().view(np.uint64)
    for j in range(A + Lk + 1):
        assert cref.fr_mont_to_ints(host[j]) == want_cols[j], j
    assert A_used >= 2


def test_k4_one_ciphertext_takes_the_power_as_the_result(eng, cref):
    """B = 1 has no tree: assert_equal_fresh compares res with the chain's last select output, whichever way the top bit goes; a weight
    of 2^W is refused on the host"""
    import torch
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import _lib

    bits, W, lb, wb = 128, 64, 10, 2
    Ln = bits // W
    n, cts, _ = _inputs(bits, 1, wb, 0x3a23)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    for weights in ([1], [2], [0], [3]):
        root = WR.wtally_trace(n, cts, weights, wb)[0]
        assert root == pow(cts[0], weights[0], n * n)
        want_a, want_l, seg = WR.wtally_cells(n, cts, weights, root, wb, bits, W, lb)
        assert seg["satisfied"]
        d_steps = _device_records(eng, cref, bits, n, cts, weights, wb)
        d_adv = torch.zeros((len(want_a), 4), dtype=torch.int64, device="cuda")
        d_lk = torch.zeros((len(want_l), 4), dtype=torch.int64, device="cuda")
        eng.circuit_expand_dev(4, Ln, W, lb, _wtally_inputs(cref, bits, n, cts, weights, root), d_steps.data_ptr(), 2 * wb, 0, d_mod.data_ptr(),
                               d_adv.data_ptr(), d_lk.data_ptr())
        eng.sync()
        assert cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64)) == want_a
        assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    with pytest.raises(pz.PzError) as e:
        eng.circuit_expand_dev(4, Ln, W, lb, _wtally_inputs(cref, bits, n, cts, [4], root), d_steps.data_ptr(), 2 * wb, 0, d_mod.data_ptr(),
                               d_adv.data_ptr(), d_lk.data_ptr())
    assert e.value.status == _lib.PZ_ERR_MESSAGE_RANGE


# ------------------------------------------------------------------------------------------------------------------ 3. structure
@pytest.mark.parametrize("shape", [S1W, S2W, (128, 64, 10, 11, 1, 1)], ids=["S1w", "S2w", "B1-W1"])
@pytest.mark.parametrize("expose", [False, True])
def test_native_structure_equals_the_python_generator(eng, shape, expose):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout, prover_native

    bits, W, lb, k, B, wb = shape
    sa = CS.stream_structure("wtally", bits, W, lb, count=B, w_bits=wb)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=expose)
    ns = prover_native.NativeStructure(eng, "wtally", bits, W, lb, k, count=B, w_bits=wb, expose=expose)
    try:
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], 2 * B * wb, B - 1)
        assert ns.starts().tolist() == starts.tolist()
        assert ns.starts()[: ns.n_adv_used + 1].tolist() == layout.break_points(WR.wtally_gate_mask(B, wb, bits, W, lb), ns.max_rows).tolist()
        assert ns.constants() == [int(c) for c in cs.constants]
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        assert (ns.n_instance, ns.n_public) == ((1, bits // W + (B + 1) * 2 * (bits // W) + B) if expose else (0, 0))
        if expose:
            assert ns.public_cells() == cs.public_cells
    finally:
        ns.free()
    for count, w_bits in ((0, wb), (65537, wb), (B, 0), (B, 65)):
        with pytest.raises(Exception):
            prover_native.NativeStructure(eng, "wtally", bits, W, lb, k, count=count, w_bits=w_bits)


# ------------------------------------------------------------------------------------------------------------------ 4. / 5. the proof
class World:
    """S1w: SRS with a known toxic scalar, both structures with the instance column, both keys, witnesses from K3 -> K4"""

    def __init__(self, eng, cref):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.bits, self.W, self.lb, self.k, self.B, self.wb = S1W
        bits, W, lb, k, B, wb = S1W
        self.n_rows = n = 1 << k
        self.nn, self.cts, self.weights = _inputs(bits, B, wb, 0x3a30)
        assert self.weights == [0, 7, 4]
        self.root = WR.wtally_trace(self.nn, self.cts, self.weights, wb)[0]
        rng = random.Random(0x3a31)
        self.s_tox = rng.randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        self.ns = prover_native.NativeStructure(eng, "wtally", bits, W, lb, k, count=B, w_bits=wb, expose=True)
        self.sa = CS.stream_structure("wtally", bits, W, lb, count=B, w_bits=wb)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)

    def statement(self, cts=None, weights=None, res=None):
        cts = self.cts if cts is None else cts
        weights = self.weights if weights is None else weights
        if res is None:
            res = WR.wtally_trace(self.nn, cts, weights, self.wb)[0]
        return WR.statement(self.nn, cts, weights, res, self.bits, self.W)

    def witness(self, cts=None, weights=None, res=None, trace=None):
        """K4's columns [m'][2^k][4] from K3's records (trace = None) or from a given trace (the forged ones: the weight cells then
        still hold `weights`)"""
        import torch

        eng, cref, ns = self.eng, self.cref, self.ns
        cts = self.cts if cts is None else cts
        weights = self.weights if weights is None else weights
        if res is None:
            res = (trace if trace is not None else WR.wtally_trace(self.nn, cts, weights, self.wb))[0]
        d_steps = _device_records(eng, cref, self.bits, self.nn, cts, weights, self.wb, trace)
        d_mod = torch.from_numpy(cref.int_to_limbs(self.nn ** 2, _words(2 * self.bits)).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        # K4 reads the chains' bits from `inputs`: a forged chain's num_to_bits must hold the exponent it was run with
        k4_weights = weights if trace is None else trace[4]
        eng.circuit_expand_cols_dev(4, self.bits // self.W, self.W, self.lb, _wtally_inputs(cref, self.bits, self.nn, cts, k4_weights, res),
                                    d_steps.data_ptr(), 2 * self.B * self.wb, self.B - 1, d_mod.data_ptr(), cols.data_ptr(),
                                    cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, self.n_rows)
        eng.sync()
        if trace is not None and list(k4_weights) != list(weights):
            # ... and the load_witness cells are put back to the weights of the statement
            pub_c, pub_r = self._weight_positions()
            for i, wv in enumerate(weights):
                cols[pub_c[i], pub_r[i]] = torch.from_numpy(cref.fr_ints_to_mont([int(wv)])[0].astype(np.int64)).cuda()
        return cols

    def _weight_positions(self):
        """(columns, rows) of the B load_witness cells: the structure's own (column, row) list of the exposed cells"""
        Ln = self.bits // self.W
        cells = self.ns.public_cells()[Ln + self.B * 2 * Ln: Ln + self.B * 2 * Ln + self.B]
        return [c for c, _ in cells], [r for _, r in cells]

    def check(self, cols, instances):
        """tally_ref.check_columns on a device-written witness under the NATIVE structure"""
        ns, cref = self.ns, self.cref
        sel, mc, mr = ns.download()
        host = cols.cpu().numpy().view(np.uint64)
        ints = [cref.fr_mont_to_ints(host[j]) for j in range(ns.m)]
        ck = ns.n_adv + ns.n_lk
        ints[ck][: ns.n_constants] = [c % R for c in ns.constants()]
        ints[ck + 1][: len(instances)] = list(instances)
        return WR.check_columns(sel, mc, mr, range(1 << self.lb), ints, ns.n_lk)

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
    inst = w.ns.gather_public(cols.data_ptr())
    assert inst == w.statement() and len(inst) == 21
    assert w.check(cols, inst) == []
    # the two keys describe one circuit
    a, b = w.key.vk_commitments(), w.pk.vk_commitments()
    assert np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])


def test_connected_proof_both_provers_two_statements_one_key(eng, cref, world):
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    good = w.statement()
    cts2, weights2 = [c ^ 0x5a5a5a for c in w.cts], [5, 0, 3]
    root2 = WR.wtally_trace(w.nn, cts2, weights2, w.wb)[0]
    other = w.statement(cts2, weights2, root2)
    assert PV.public_inputs("wtally", w.nn, None, w.root, cts=w.cts, weights=w.weights, enc_bits=w.bits, limb_bits=w.W) == good != other
    seeds = [b"wtally-stepper", b"wtally-python", b"wtally-second"]
    cols = w.witness()
    p0 = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seeds[0]), seed=5, instances=good)
    p1 = prover.create_proof(w.pk, w.witness(), prover.HashTranscript(seeds[1]), seed=6, tile=8, instances=good)
    cols2 = w.witness(cts2, weights2)
    assert w.ns.gather_public(cols2.data_ptr()) == other
    p2 = prover_native.create_proof(w.key, cols2.data_ptr(), prover.HashTranscript(seeds[2]), seed=7, instances=other)       # the SAME key
    proofs, inst = [p0, p1, p2], [good, good, other]
    for pr, seed, st in zip(proofs, seeds, inst):
        assert _oracle_checks(cref, w, pr, seed, st) == (True, True, True)
    assert PV.verify_batch(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=inst) == (True, [True, True, True])          # pz_verify_batch_pub
    wire = [PV.proof_to_bytes(eng, w.vk, p) for p in proofs]
    assert all(len(b) == PV.proof_size_bytes(w.vk) for b in wire)
    assert PV.verify_batch_bytes(eng, w.params, w.vk, wire, seeds, instances=inst) == (True, [True, True, True])
    assert PV.proof_to_bytes(eng, w.vk, PV.proof_from_bytes(eng, w.vk, wire[0])) == wire[0]
    # ---- 6 (a), (b): the statement alone changed -- a weight by one, a ciphertext limb
    Ln = w.bits // w.W
    L = 2 * Ln
    for at in (Ln + w.B * L + 1, Ln + 2 * L + 1):        # w_2; one limb of c_3
        bad = [list(s) for s in inst]
        bad[0][at] += 1
        assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=bad) == (False, [False, True, True])
        assert PV.verify_batch(eng, w.params, w.vk, proofs, seeds, instances=bad) == (False, [False, True, True])
    # the statements of two different tallies swapped
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[other, good, good]) == (False, [False, True, False])


FORGES = [("weight", 1, 6), ("tree", 0, "a", 1), ("leaf", 2, 1)]


@pytest.mark.parametrize("forge", FORGES, ids=["chain-run-with-another-weight", "tree-operand-is-power+1", "first-sq-is-c+1"])
def test_forged_edges_are_rejected(eng, cref, world, forge):
    """6 (c), (d), (e): chain 2 run consistently with w' = 6 while the statement (and the weight's cell) says 7; the first tree record
    recomputed with a' = power_1 + 1; chain 3's first sq taken as c_3 + 1 -- each with everything downstream and res recomputed
    consistently, so every gate, every lookup and the final equality hold and only a copy constraint can object (the weight cell's, the
    power -> tree ties, the leaf tie) -- and the proof is rejected"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    ftrace = WR.wtally_trace(w.nn, w.cts, w.weights, w.wb, forge=forge)
    froot = ftrace[0]
    assert froot != w.root
    inst = w.statement(res=froot)
    cols = w.witness(trace=ftrace)
    assert w.ns.gather_public(cols.data_ptr()) == inst
    bad = w.check(cols, inst)
    assert bad and {t for t, _, _ in bad} == {"copy"}
    honest, hinst = w.witness(), w.statement()
    assert w.check(honest, hinst) == []
    seed = b"wtally-forged"
    pf = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=inst)
    ph = prover_native.create_proof(w.key, honest.data_ptr(), prover.HashTranscript(seed), seed=9, instances=hinst)
    assert not pf.h_degree_ok and ph.h_degree_ok
    assert PV.verify_batch_native(eng, w.params, w.vk, [pf, ph], [seed, seed], instances=[inst, hinst]) == (False, [False, True])
    pf2 = prover.create_proof(w.pk, w.witness(trace=ftrace), prover.HashTranscript(seed), seed=9, tile=8, instances=inst)
    assert PV.verify_batch_native(eng, w.params, w.vk, [pf2], [seed], instances=[inst]) == (False, [False])
