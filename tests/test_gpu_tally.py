"""GPU: the tally circuit (kind 3 / "tally") through every layer -- the product tree (K3), the cell stream (K4),
the native structure generator, and ONE connected proof with the statement "C is the product of exactly these c_1 .. c_B under n" by
both provers -- against the independent restatement of tests/tally_ref.py in Python integers.  Every comparison is exact.

Main shape S1: 128-bit n, 64-bit limbs, lookup_bits 10, k = 11, B = 5 -- four advice columns (break points are crossed), an odd B
(the carried element on two levels), 26 public values."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import public_ref as PR
from tests import tally_ref as TR

pytestmark = pytest.mark.gpu

R = P.FR_R
BF = 6
S1 = (128, 64, 10, 11, 5)
S2 = (264, 88, 11, 12, 3)       # the reference's add-test key on 88-bit limbs (paillier.rs:186-187)


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def _inputs(bits, B, seed):
    rng = random.Random(seed)
    n = P.synth_paillier_inputs(bits, seed)[0]
    return n, [rng.randrange(1, n * n) for _ in range(B)]


def _words(bits):
    return -(-bits // 64)


# ------------------------------------------------------------------------------------------------------------------ 1. K3
@pytest.mark.parametrize("bits,B", [(128, 2), (128, 5), (128, 6), (128, 7), (128, 1000), (264, 3), (2048, 9), (3072, 5)])
def test_k3_tree_records_equal_the_reference(eng, cref, bits, B):
    n, cts = _inputs(bits, B, 0x7a20 + B)
    Ln = _words(bits)
    L = 2 * Ln
    lim = cref.int_to_limbs
    c, steps = eng.paillier_tally(Ln, lim(n, Ln), np.stack([lim(v, L) for v in cts]))
    root, want = TR.tally_trace(n, cts)
    assert steps.shape == (B - 1, 4, L) and cref.limbs_to_int(c) == root
    for t, st in enumerate(want):
        assert tuple(cref.limbs_to_int(steps[t, f]) for f in range(4)) == st, t
    c2, none = eng.paillier_tally(Ln, lim(n, Ln), np.stack([lim(v, L) for v in cts]), want_steps=False)
    assert none is None and np.array_equal(c2, c)
    if B == 2:
        q, r = eng.mul_mod(L, lim(cts[0], L), lim(cts[1], L), lim(n * n, L))
        assert np.array_equal(steps[0, 2], q) and np.array_equal(steps[0, 3], r)


def test_k3_refusals(eng, cref):
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import _lib

    n, cts = _inputs(128, 5, 0x7a21)
    lim = cref.int_to_limbs
    arr = lambda vs: np.stack([lim(v, 4) for v in vs])
    for bad in (0, 2, 4):          # an operand of level 0, another, and the carried one: a ciphertext EQUAL to n^2
        vs = list(cts)
        vs[bad] = n * n
        with pytest.raises(pz.PzError) as e:
            eng.paillier_tally(2, lim(n, 2), arr(vs))
        assert e.value.status == _lib.PZ_ERR_RANGE
    with pytest.raises(pz.PzError) as e:
        eng.paillier_tally(2, lim(0, 2), arr(cts))
    assert e.value.status == _lib.PZ_ERR_ZERO_MODULUS
    with pytest.raises(pz.PzError) as e:
        eng.paillier_tally(2, lim(n, 2), arr(cts[:1]))
    assert e.value.status == _lib.PZ_ERR_INVALID
    out = np.zeros(4, dtype=np.uint64)
    steps = np.zeros((3, 4, 4), dtype=np.uint64)
    a = arr(cts)
    rc = eng.L.pz_paillier_tally(eng.ctx, 2, 5, lim(n, 2).ctypes.data, a.ctypes.data, steps.ctypes.data, 3, out.ctypes.data)
    assert rc == _lib.PZ_ERR_CAPACITY
    # the context still serves an honest call
    c, _ = eng.paillier_tally(2, lim(n, 2), arr(cts))
    assert cref.limbs_to_int(c) == TR.tally_trace(n, cts)[0]


# ------------------------------------------------------------------------------------------------------------------ 2. K4
def _device_records(eng, cref, bits, n, cts, steps=None):
    """the B - 1 records on the device, fields of ceil(2 bits / 64) words: K3's own (steps = None), or given ones (the forged traces)"""
    import torch

    Ln, L64 = _words(bits), _words(2 * bits)
    lim = cref.int_to_limbs
    if steps is None:
        c, rec = eng.paillier_tally(Ln, lim(n, Ln), np.stack([lim(v, 2 * Ln) for v in cts]))
        assert cref.limbs_to_int(c) == TR.tally_trace(n, cts)[0] and not rec[:, :, L64:].any()
        rec = np.ascontiguousarray(rec[:, :, :L64])
    else:
        rec = np.stack([np.stack([lim(v, L64) for v in st]) for st in steps])
    return torch.from_numpy(rec.astype(np.int64)).cuda()


def _tally_inputs(cref, bits, n, cts, res):
    lim = cref.int_to_limbs
    return np.concatenate([lim(n, _words(bits))] + [lim(v, _words(2 * bits)) for v in list(cts) + [res]])


@pytest.mark.parametrize("shape", [S1, S2])
def test_k4_dense_stream_and_break_point_columns_equal_the_reference(eng, cref, shape):
    import torch
    from paillier_halo2_amd import layout

    bits, W, lb, k, B = shape
    Ln, n_rows = bits // W, 1 << k
    n, cts = _inputs(bits, B, 0x7a22)
    root, _ = TR.tally_trace(n, cts)
    want_a, want_l, _ = TR.tally_cells(n, cts, root, bits, W, lb)
    na, nl = eng.circuit_cells(3, Ln, W, lb, B - 1, 0)
    assert (na, nl) == (len(want_a), len(want_l))
    d_steps = _device_records(eng, cref, bits, n, cts)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    inputs = _tally_inputs(cref, bits, n, cts, root)
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.circuit_expand_dev(3, Ln, W, lb, inputs, d_steps.data_ptr(), B - 1, 0, d_mod.data_ptr(), d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d" % (len(bad), bad[0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l
    # ---- the same stream in break-point columns
    rb = layout.row_budget(k)
    starts = layout.break_points(TR.tally_gate_mask(B, bits, W, lb), rb.max_rows)
    A_used = starts.shape[0] - 1
    A, Lk = rb.columns_for(na, filled=A_used), rb.columns_for(nl)
    full = np.concatenate([starts, np.full(A - A_used, na, dtype=np.uint64)])
    d_starts = torch.from_numpy(full.astype(np.int64)).cuda()
    cols = torch.zeros((A + Lk + 1, n_rows, 4), dtype=torch.int64, device="cuda")
    eng.circuit_expand_cols_dev(3, Ln, W, lb, inputs, d_steps.data_ptr(), B - 1, 0, d_mod.data_ptr(), cols.data_ptr(), cols[A].data_ptr(),
                                d_starts.data_ptr(), A, rb.max_rows, rb.max_rows, n_rows)
    eng.sync()
    want_cols = TR.place(want_a, want_l, full, A, Lk, rb.max_rows, k, [])
    host = cols.cpu().numpy().view(np.uint64)
    for j in range(A + Lk + 1):
        assert cref.fr_mont_to_ints(host[j]) == want_cols[j], j
    if shape == S1:
        assert A_used >= 2


def test_k4_dense_stream_of_a_mismatching_result_equals_the_reference(eng, cref):
    """the claimed result differs from the root in a middle limb only: the running-equality chain drops there and stays down, the
    is_zero inverse cell of that limb is a true inverse -- the cells the matching streams above never reach"""
    import torch

    bits, W, lb, B = 128, 64, 10, 2
    Ln = bits // W
    n, cts = _inputs(bits, B, 0x7a23)
    root, _ = TR.tally_trace(n, cts)
    res = root ^ (1 << (W + 5))                 # limb 1 of 4
    want_a, want_l, seg = TR.tally_cells(n, cts, res, bits, W, lb)
    assert not seg["satisfied"]
    na, nl = eng.circuit_cells(3, Ln, W, lb, B - 1, 0)
    assert (na, nl) == (len(want_a), len(want_l))
    d_steps = _device_records(eng, cref, bits, n, cts)
    d_mod = torch.from_numpy(cref.int_to_limbs(n * n, _words(2 * bits)).astype(np.int64)).cuda()
    d_adv = torch.zeros((na, 4), dtype=torch.int64, device="cuda")
    d_lk = torch.zeros((nl, 4), dtype=torch.int64, device="cuda")
    eng.circuit_expand_dev(3, Ln, W, lb, _tally_inputs(cref, bits, n, cts, res), d_steps.data_ptr(), B - 1, 0, d_mod.data_ptr(),
                           d_adv.data_ptr(), d_lk.data_ptr())
    eng.sync()
    got_a = cref.fr_mont_to_ints(d_adv.cpu().numpy().view(np.uint64))
    bad = [i for i, (x, y) in enumerate(zip(got_a, want_a)) if x != y]
    assert not bad, "%d advice cells differ, first at %d (assert_equal at %d)" % (len(bad), bad[0], seg["assert_equal"][0])
    assert cref.fr_mont_to_ints(d_lk.cpu().numpy().view(np.uint64)) == want_l


# ------------------------------------------------------------------------------------------------------------------ 3. structure
@pytest.mark.parametrize("shape", [S1, S2])
@pytest.mark.parametrize("expose", [False, True])
def test_native_structure_equals_the_python_generator(eng, shape, expose):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout, prover_native

    bits, W, lb, k, B = shape
    sa = CS.stream_structure("tally", bits, W, lb, count=B)
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=expose)
    ns = prover_native.NativeStructure(eng, "tally", bits, W, lb, k, count=B, expose=expose)
    try:
        assert (ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.m) == (cs.n_adv, cs.n_adv_used, cs.n_lk, cs.max_rows, cs.m)
        assert (ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r) == (sa.n_cells, sa.lookup_src.shape[0], B - 1, 0)
        assert ns.starts().tolist() == starts.tolist()
        assert ns.starts()[: ns.n_adv_used + 1].tolist() == layout.break_points(TR.tally_gate_mask(B, bits, W, lb), ns.max_rows).tolist()
        assert ns.constants() == [int(c) for c in cs.constants]
        sel, mc, mr = ns.download()
        assert np.array_equal(sel, cs.selectors)
        assert np.array_equal(mc, cs.map_col.view(np.uint32)) and np.array_equal(mr, cs.map_row.view(np.uint32))
        assert (ns.n_instance, ns.n_public) == ((1, bits // W + (B + 1) * 2 * (bits // W)) if expose else (0, 0))
        if expose:
            assert ns.public_cells() == cs.public_cells
    finally:
        ns.free()
    with pytest.raises(Exception):
        prover_native.NativeStructure(eng, "tally", bits, W, lb, k, count=1)


# ------------------------------------------------------------------------------------------------------------------ 4. / 5. the proof
class World:
    """S1: SRS with a known toxic scalar, both structures with the instance column, both keys, witnesses from K3 -> K4"""

    def __init__(self, eng, cref):
        import torch
        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.bits, self.W, self.lb, self.k, self.B = S1
        bits, W, lb, k, B = S1
        self.n_rows = n = 1 << k
        self.nn, self.cts = _inputs(bits, B, 0x7a30)
        self.root, self.steps = TR.tally_trace(self.nn, self.cts)
        rng = random.Random(0x7a31)
        self.s_tox = rng.randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        self.ns = prover_native.NativeStructure(eng, "tally", bits, W, lb, k, count=B, expose=True)
        self.sa = CS.stream_structure("tally", bits, W, lb, count=B)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)

    def witness(self, cts=None, res=None, steps=None):
        """K4's columns [m'][2^k][4] from K3's records (steps = None) or from given records (the forged traces)"""
        import torch

        eng, cref, ns = self.eng, self.cref, self.ns
        cts = self.cts if cts is None else cts
        if res is None:
            res = TR.tally_trace(self.nn, cts)[0]
        d_steps = _device_records(eng, cref, self.bits, self.nn, cts, steps)
        d_mod = torch.from_numpy(cref.int_to_limbs(self.nn ** 2, _words(2 * self.bits)).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, self.n_rows, 4), dtype=torch.int64, device="cuda")
        eng.circuit_expand_cols_dev(3, self.bits // self.W, self.W, self.lb, _tally_inputs(cref, self.bits, self.nn, cts, res), d_steps.data_ptr(),
                                    self.B - 1, 0, d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv,
                                    ns.max_rows, ns.max_rows, self.n_rows)
        eng.sync()
        return cols

    def check(self, cols, instances):
        """tally_ref.check_columns on a device-written witness under the NATIVE structure"""
        ns, cref = self.ns, self.cref
        sel, mc, mr = ns.download()
        host = cols.cpu().numpy().view(np.uint64)
        ints = [cref.fr_mont_to_ints(host[j]) for j in range(ns.m)]
        ck = ns.n_adv + ns.n_lk
        ints[ck][: ns.n_constants] = [c % R for c in ns.constants()]
        ints[ck + 1][: len(instances)] = list(instances)
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
    assert inst == TR.statement(w.nn, w.cts, w.root, w.bits, w.W) and len(inst) == 26
    assert w.check(cols, inst) == []
    # the two keys describe one circuit
    a, b = w.key.vk_commitments(), w.pk.vk_commitments()
    assert np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])


def test_connected_proof_both_provers_two_tallies_one_key(eng, cref, world):
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    good = TR.statement(w.nn, w.cts, w.root, w.bits, w.W)
    cts2 = [c ^ 0x5a5a5a for c in w.cts]
    root2 = TR.tally_trace(w.nn, cts2)[0]
    other = TR.statement(w.nn, cts2, root2, w.bits, w.W)
    assert PV.public_inputs("tally", w.nn, None, w.root, cts=w.cts, enc_bits=w.bits, limb_bits=w.W) == good != other
    seeds = [b"tally-stepper", b"tally-python", b"tally-second"]
    cols = w.witness()
    p0 = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seeds[0]), seed=5, instances=good)
    p1 = prover.create_proof(w.pk, w.witness(), prover.HashTranscript(seeds[1]), seed=6, tile=8, instances=good)
    cols2 = w.witness(cts2)
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
    # ---- 5 (a), (b): the statement alone changed
    L = 2 * (w.bits // w.W)
    for at in (len(good) - 1, 2 + 2 * L + 1):            # one limb of the claimed C; one limb of c_3
        bad = [list(s) for s in inst]
        bad[0][at] += 1
        assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=bad) == (False, [False, True, True])
        assert PV.verify_batch(eng, w.params, w.vk, proofs, seeds, instances=bad) == (False, [False, True, True])
    # the statements of two different tallies swapped
    assert PV.verify_batch_native(eng, w.params, w.vk, proofs, seeds, instances=[other, good, good]) == (False, [False, True, False])


@pytest.mark.parametrize("forge", [(5 // 2, "a", 1), (0, "b", 1)], ids=["interior-edge", "leaf-edge"])
def test_forged_tree_edges_are_rejected(eng, cref, world, forge):
    """5 (c), (d): a record recomputed with a' = r_0 + 1 (the first level-1 block) or b' = c_2 + 1 (level 0, c_2's assignment kept),
    everything downstream and res recomputed consistently: every gate, every lookup and the final equality hold, so only the tree's
    copy constraints can object -- and the proof is rejected"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    w = world
    froot, fsteps = TR.tally_trace(w.nn, w.cts, forge=forge)
    assert froot != w.root
    inst = TR.statement(w.nn, w.cts, froot, w.bits, w.W)
    cols = w.witness(res=froot, steps=fsteps)
    assert w.ns.gather_public(cols.data_ptr()) == inst
    bad = w.check(cols, inst)
    assert bad and {t for t, _, _ in bad} == {"copy"}
    honest = w.witness()
    assert w.check(honest, TR.statement(w.nn, w.cts, w.root, w.bits, w.W)) == []
    seed = b"tally-forged"
    pf = prover_native.create_proof(w.key, cols.data_ptr(), prover.HashTranscript(seed), seed=9, instances=inst)
    ph = prover_native.create_proof(w.key, honest.data_ptr(), prover.HashTranscript(seed), seed=9,
                                    instances=TR.statement(w.nn, w.cts, w.root, w.bits, w.W))
    assert not pf.h_degree_ok and ph.h_degree_ok
    got = PV.verify_batch_native(eng, w.params, w.vk, [pf, ph], [seed, seed], instances=[inst, TR.statement(w.nn, w.cts, w.root, w.bits, w.W)])
    assert got == (False, [False, True])
    pf2 = prover.create_proof(w.pk, w.witness(res=froot, steps=fsteps), prover.HashTranscript(seed), seed=9, tile=8, instances=inst)
    assert PV.verify_batch_native(eng, w.params, w.vk, [pf2], [seed], instances=[inst]) == (False, [False])


# ------------------------------------------------------------------------------------------------------------------ 6. regression guard
def test_kind1_structure_and_proof_are_unchanged(eng, cref):
    """the add circuit (kind 1) at 128-bit / k = 12: its structure arrays and one seeded proof's wire bytes, by digest, as the library
    produced them before the tally existed (tests/golden/tally_kind1_regression.json)"""
    import json
    import os

    from tests import tally_kind1_digest as KD

    with open(os.path.join(os.path.dirname(__file__), "golden", "tally_kind1_regression.json")) as f:
        want = json.load(f)
    assert KD.digests(eng, cref) == want
