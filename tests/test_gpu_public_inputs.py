"""GPU: public inputs -- one instance column carried from the circuit structure through keygen, both provers, the verifiers and the wire
path (include/pz.h "PUBLIC INPUTS"; csrc/pz_public.hip), against the reference in Python integers
(tests/public_ref.py over the unmodified oracle).  Three shapes: encrypt 128 / 64 / k 14 (m' = 35, a last product set of one column),
add 128 / 64 / k 12 (m' = 4, a full pair), encrypt_uniform 128 / 64 / k 15 (m' = 21).  Every comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import public_ref as PR

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


class World:
    """one shape: the reference (built once), SRS, both structures, both keys, the witness"""

    def __init__(self, eng, cref, shape):
        import torch

        from paillier_halo2_amd import circuit_structure as CS
        from paillier_halo2_amd import prover, prover_native, srs
        from paillier_halo2_amd import verifier as PV

        self.eng, self.cref = eng, cref
        self.kind, self.bits, self.W, self.k, self.lb, seed = shape
        kind, bits, W, k, lb = shape[:5]
        self.n = n = 1 << k
        self.Ln = Ln = bits // W
        self.inp = PR.inputs(kind, bits, seed)
        nn, g, x, y, res = self.inp
        self.ref_st = PR.CQ.build(kind, nn, g, x, y, res, bits, W, lb, k)
        self.cells = PR.exposed_positions(kind, nn, g, x, y, res, bits, W, lb)
        self.statement = PR.statement(kind, nn, g, x, y, res, bits, W)
        rng = random.Random(0x9b1 + k)
        self.s_tox = rng.randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        g2, s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)
        self.ns = prover_native.NativeStructure(eng, kind, bits, W, lb, k, exp_g=x, exp_r=nn, expose=True)
        self.sa = CS.stream_structure(kind, bits, W, lb, x, nn)
        self.cs, self.starts = CS.columns(self.sa, k, lb, device="cpu", expose=True)
        self.key = self.ns.key(self.bl, self.bm, tile=8)
        self.pk = prover.keygen(eng, self.cs, self.bl, self.bm)
        self.vk = PV.VerifyingKey.from_proving_key(self.pk)
        self._proofs = None

    def witness(self, inp=None):
        """the K4 columns [m'][2^k][4] of the circuit for inputs `inp` (default: the shape's own)"""
        import torch

        eng, cref, Ln, W, lb, n, ns = self.eng, self.cref, self.Ln, self.W, self.lb, self.n, self.ns
        nn, g, x, y, res = inp or self.inp
        arr = lambda v, l: cref.int_to_limbs(v, l)
        L = 2 * Ln
        kid = PR.KIND_ID[self.kind]
        if self.kind == "add":
            q, rem = eng.mul_mod(L, arr(x, L), arr(y, L), arr(nn * nn, L))
            assert cref.limbs_to_int(rem) == res
            d_steps = torch.from_numpy(np.stack([arr(x, L), arr(y, L), q, rem]).astype(np.int64)).cuda().view(1, 4, L)
        else:
            cap = ns.n_steps_g + ns.n_steps_r + 1
            d_steps = torch.zeros((cap, 4, L), dtype=torch.int64, device="cuda")
            if self.kind == "encrypt":
                c, _, _ = eng.paillier_encrypt_dev(Ln, arr(nn, Ln), arr(g, Ln), arr(x, Ln), arr(y, Ln), d_steps.data_ptr(), cap)
            else:
                c, _, _ = eng.paillier_encrypt_uniform_dev(Ln, self.bits, arr(nn, Ln), arr(g, Ln), arr(x, Ln), arr(y, Ln), d_steps.data_ptr(), cap)
            assert cref.limbs_to_int(c[0]) == res
        d_mod = torch.from_numpy(arr(nn * nn, L).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, n, 4), dtype=torch.int64, device="cuda")
        inputs = np.concatenate([arr(nn, Ln), arr(g, Ln), arr(x, Ln), arr(y, Ln), arr(res, L)])
        eng.circuit_expand_cols_dev(kid, Ln, W, lb, inputs, d_steps.data_ptr(), ns.n_steps_g, ns.n_steps_r, d_mod.data_ptr(), cols.data_ptr(),
                                    cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, n)
        eng.sync()
        return cols

    def proofs(self):
        """(stepper proof, prover.py proof), their seeds, the gathered statement -- made once"""
        from paillier_halo2_amd import prover, prover_native

        if self._proofs is None:
            cols = self.witness()
            gathered = self.ns.gather_public(cols.data_ptr())
            s0, s1 = b"pub-stepper-" + self.kind.encode(), b"pub-python-" + self.kind.encode()
            p0 = prover_native.create_proof(self.key, cols.data_ptr(), prover.HashTranscript(s0), seed=5, instances=gathered)
            p1 = prover.create_proof(self.pk, self.witness(), prover.HashTranscript(s1), seed=6, tile=8, instances=gathered)
            self._proofs = ([p0, p1], [s0, s1], gathered)
        return self._proofs

    def close(self):
        self.key.free()
        self.ns.free()
        self.bl.free()
        self.bm.free()


@pytest.fixture(scope="module")
def worlds(eng, cref):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = World(eng, cref, next(s for s in PR.SHAPES if s[0] == kind))
        return made[kind]

    yield get
    for w in made.values():
        w.close()


KINDS = [s[0] for s in PR.SHAPES]


# ------------------------------------------------------------------------------------------------------------------ 4. structure
@pytest.mark.parametrize("kind", KINDS)
def test_exposed_structure_equals_the_reference(eng, worlds, kind):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import prover_native

    w = worlds(kind)
    ns, cs, st = w.ns, w.cs, w.ref_st
    expect_m = {"encrypt": (34, 35, 18), "add": (3, 4, 2), "encrypt_uniform": (20, 21, 11)}[kind]
    assert (st.m, ns.m, -(-ns.m // 2)) == expect_m and cs.m == ns.m and (ns.n_instance, ns.n_public) == (1, len(w.cells))
    assert ns.public_cells() == [st.pos(c) for c in w.cells] == cs.public_cells
    want_c, want_r = PR.reference_maps(st, w.cells, ns.constants())
    sel, mc, mr = ns.download()
    assert mc.shape == (st.m + 1, w.n) and np.array_equal(mc, want_c) and np.array_equal(mr, want_r)
    assert [int(c) for c in cs.constants] == ns.constants()
    assert np.array_equal(cs.map_col.view(np.uint32), want_c) and np.array_equal(cs.map_row.view(np.uint32), want_r)
    # selectors and every other output are those of the unexposed structure
    nn, g, x, y, res = w.inp
    plain = prover_native.NativeStructure(eng, kind, w.bits, w.W, w.lb, w.k, exp_g=x, exp_r=nn)
    try:
        assert (plain.n_instance, plain.n_public, plain.m) == (0, 0, st.m)
        sel0, mc0, mr0 = plain.download()
        assert np.array_equal(sel, sel0) and np.array_equal(sel, cs.selectors) and np.array_equal(sel, st.selectors)
        assert plain.starts().tolist() == ns.starts().tolist() == w.starts.tolist() and plain.constants() == ns.constants()
        for f in ("n_adv", "n_adv_used", "n_lk", "max_rows", "n_constants", "n_cells", "n_lookups", "n_steps_g", "n_steps_r"):
            assert getattr(plain, f) == getattr(ns, f), f
        moved = (mc[:st.m] != mc0) | (mr[:st.m] != mr0)
        assert int(moved.sum()) == len(w.cells) and (mc[:st.m][moved] == st.m).all()
        assert eng.L.pz_structure_expose(plain.handle) == 0 and eng.L.pz_structure_expose(plain.handle) == -1      # once per structure
    finally:
        plain.free()


# ------------------------------------------------------------------------------------------------------------------ 5. k_instance_eval
def _instance_eval_dev(eng, cref, k, vals, xs):
    """B proofs x L canonical values, B challenges -> (results as integers, flags)"""
    import torch

    B, L = len(xs), len(vals[0])
    words = np.zeros((B, max(L, 1), 4), dtype=np.uint64)
    for b in range(B):
        for i, v in enumerate(vals[b]):
            for j in range(4):
                words[b, i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    d_inst = torch.from_numpy(words.view(np.int64)).cuda()
    d_x = torch.from_numpy(np.asarray(cref.fr_ints_to_mont(xs), dtype=np.uint64).view(np.int64)).cuda()
    d_out = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
    d_fl = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    om = np.asarray(cref.fr_ints_to_mont([P.fr_omega(k)])[0], dtype=np.uint64)
    ninv = np.asarray(cref.fr_ints_to_mont([pow(1 << k, -1, R)])[0], dtype=np.uint64)
    eng.sync()
    eng._chk(eng.L.pz_instance_eval_dev(eng.ctx, k, om.ctypes.data, ninv.ctypes.data, d_inst.data_ptr(), L, B, d_x.data_ptr(), d_out.data_ptr(),
                                        d_fl.data_ptr()), "pz_instance_eval_dev")
    eng.sync()
    return cref.fr_mont_to_ints(d_out.cpu().numpy().view(np.uint64)), d_fl.cpu().numpy().tolist()


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("L", (1, 2, 63, 64, 65, 255, 256, 257, (1 << 10) - (BF + 1)))
def test_instance_eval_kernel_against_python_integers(eng, cref, L, B):
    k = 10
    rng = random.Random(0x1e57 + 31 * L + B)
    vals = [[rng.randrange(R) for _ in range(L)] for _ in range(B)]
    xs = [rng.randrange(2, R) for _ in range(B)]
    got, flags = _instance_eval_dev(eng, cref, k, vals, xs)
    assert flags == [0] * B
    assert got == [PR.instance_eval(k, vals[b], xs[b]) for b in range(B)]


def test_instance_eval_kernel_k14_domain_point_and_range(eng, cref):
    rng = random.Random(0x1e58)
    k = 14
    vals = [[rng.randrange(R) for _ in range(8)]]
    xs = [rng.randrange(2, R)]
    assert _instance_eval_dev(eng, cref, k, vals, xs) == ([PR.instance_eval(k, vals[0], xs[0])], [0])
    # more than one workgroup per proof (1024 rows each), a length that is no multiple of it, the largest row the circuits can use
    k = 12
    L = (1 << k) - (BF + 1)
    vals = [[rng.randrange(R) for _ in range(L)] for _ in range(2)]
    xs = [rng.randrange(2, R) for _ in range(2)]
    got, flags = _instance_eval_dev(eng, cref, k, vals, xs)
    assert flags == [0, 0] and got == [PR.instance_eval(k, vals[b], xs[b]) for b in range(2)]
    # a challenge on the domain sets bit 0 of its proof's flag only -- hit (row 5 < L) or not (L = 1: x^n = 1 alone says so);
    # a value >= r sets bit 1
    k = 10
    w5 = pow(P.fr_omega(k), 5, R)
    vals = [[rng.randrange(R) for _ in range(9)] for _ in range(3)]
    xs = [rng.randrange(2, R), w5, rng.randrange(2, R)]
    got, flags = _instance_eval_dev(eng, cref, k, vals, xs)
    assert flags == [0, 1, 0] and got[0] == PR.instance_eval(k, vals[0], xs[0]) and got[2] == PR.instance_eval(k, vals[2], xs[2])
    assert _instance_eval_dev(eng, cref, k, [[7]], [w5])[1] == [1]
    vals[2][4] = R
    vals[0][8] = (1 << 256) - 1
    assert _instance_eval_dev(eng, cref, k, vals, [xs[0], xs[2], xs[2]])[1] == [2, 0, 2]


# ------------------------------------------------------------------------------------------------------------------ 6. keygen
def test_keygen_with_the_instance_column(eng, cref, worlds):
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    for kind in KINDS:
        w = worlds(kind)
        vk_native = w.key.vk_commitments()
        got = PV.VerifyingKey.from_structure(eng, w.ns, w.bl, tile=8)                       # pz_vk_keygen_pub_dev
        assert (got.n_instance, got.n_public, got.m, got.n_sets) == (1, len(w.cells), w.ns.m, -(-w.ns.m // 2))
        assert got.sigma.shape == (w.ns.m, 8) and np.array_equal(got.fixed, vk_native["fixed"]) and np.array_equal(got.sigma, vk_native["sigma"])
        assert np.array_equal(w.vk.sigma, got.sigma) and np.array_equal(w.vk.fixed, got.fixed)      # prover.py's key on the Python structure
        host = PV.VerifyingKey.from_structure(eng, w.cs, w.bl, tile=3)                      # pz_vk_keygen_pub (host arrays)
        assert np.array_equal(host.sigma, got.sigma) and np.array_equal(host.fixed, got.fixed)
    # the add shape: the sigma commitments by the oracle's C MSM from the REFERENCE map
    w = worlds("add")
    st = w.ref_st
    want_c, want_r = PR.reference_maps(st, w.cells, w.ns.constants())
    omega, delta = P.fr_omega(w.k), prover.DELTA
    wp = [1] * w.n
    for i in range(1, w.n):
        wp[i] = wp[i - 1] * omega % R
    bases = w.d_gl.cpu().numpy().view(np.uint64)
    for j in range(st.m + 1):
        sig = [pow(delta, int(want_c[j, i]), R) * wp[int(want_r[j, i])] % R for i in range(w.n)]
        pt = cref.g1_normalize(cref.msm_g1(cref.fr_ints_to_mont(sig), bases))
        assert np.array_equal(np.asarray(pt).reshape(8), w.key.vk_commitments()["sigma"][j]), j
    # n_instance = 0 through the _pub entry points IS the old entry point: the same commitments and, for one seeded proof, the same words
    nn, g, x, y, res = w.inp
    plain = prover_native.NativeStructure(eng, "add", w.bits, w.W, w.lb, w.k, exp_g=x, exp_r=nn)
    h_old = C.c_void_p()
    try:
        key_pub = plain.key(w.bl, w.bm, tile=8)                                             # pz_pk_create_pub_dev(.., 0, 0, ..)
        eng._chk(eng.L.pz_pk_create_dev(eng.ctx, w.bl.handle, w.bm.handle, plain.k, plain.lookup_bits, BF, plain.max_rows, plain.n_adv, plain.n_lk,
                                        C.c_void_p(plain.d_selectors), C.c_void_p(plain._constants), plain.n_constants, C.c_void_p(plain.d_map_col),
                                        C.c_void_p(plain.d_map_row), 8, (1 << 64) - 1, C.byref(h_old)), "pz_pk_create_dev")
        key_old = prover_native.NativeKey.__new__(prover_native.NativeKey)
        key_old.eng, key_old.st, key_old.handle = eng, key_pub.st, h_old
        key_old.n_fixed, key_old.m, key_old.n_sets, key_old.blinding_words, key_old.evals_words = (key_pub.n_fixed, key_pub.m, key_pub.n_sets,
                                                                                                  key_pub.blinding_words, key_pub.evals_words)
        a, b = key_pub.vk_commitments(), key_old.vk_commitments()
        assert key_pub.m == st.m and np.array_equal(a["fixed"], b["fixed"]) and np.array_equal(a["sigma"], b["sigma"])
        fx, sg = eng.vk_keygen_dev(w.bl, plain.k, plain.lookup_bits, plain.n_adv, plain.n_lk, plain.d_selectors, plain.constants(), plain.d_map_col,
                                   plain.d_map_row, 8)
        assert np.array_equal(fx, a["fixed"]) and np.array_equal(sg, a["sigma"])
        cols = w.witness()[:st.m].contiguous()
        ch = prover.Challenges(*(random.Random(4).randrange(2, R) for _ in range(8)))
        p_pub = prover_native.create_proof(key_pub, cols.clone().data_ptr(), ch, seed=9)
        p_old = prover_native.create_proof(key_old, cols.clone().data_ptr(), ch, seed=9)
        for nm in p_pub.commitments:
            assert np.array_equal(p_pub.commitments[nm], p_old.commitments[nm]), nm
        for nm in p_pub.evals:
            assert np.array_equal(p_pub.evals[nm], p_old.evals[nm]), nm
        key_pub.free()
        key_old.free()
    finally:
        plain.free()


# ------------------------------------------------------------------------------------------------------------------ 7. proofs
@pytest.mark.parametrize("kind", KINDS)
def test_proofs_with_a_statement_verify_everywhere(eng, cref, worlds, kind):
    from oracle import verifier as V
    from paillier_halo2_amd import prover
    from paillier_halo2_amd import verifier as PV

    w = worlds(kind)
    proofs, seeds, gathered = w.proofs()
    nn, g, x, y, res = w.inp
    want = PV.public_inputs(kind, nn, g, res, x, y, enc_bits=w.bits, limb_bits=w.W) if kind == "add" else \
        PV.public_inputs(kind, nn, g, res, enc_bits=w.bits, limb_bits=w.W)
    assert gathered == want == w.statement
    vk, A, Lk, m, S = w.vk, w.ns.n_adv, w.ns.n_lk, w.ns.m, -(-w.ns.m // 2)
    assert PV.proof_size_bytes(vk) == 32 * (A + 4 * Lk + S + 6 + 4 * A + (Lk + 1) + (A + 2) + m + 3 * S + 5 * Lk + 1)
    vk_c = w.key.vk_commitments()
    for pr, seed in zip(proofs, seeds):
        assert pr.h_degree_ok
        ev = {f: PR.ints_of(cref, v) for f, v in pr.evals.items()}
        assert len(ev["sigma"]) == m and len(ev["perm_z"]) == S
        ch = PR.replay_challenges_pub(seed, gathered, pr.commitments, pr.evals)
        assert ch != V.replay_challenges(seed, pr.commitments, pr.evals)                       # the statement is in the transcript
        inst_x = PR.instance_eval(w.k, gathered, ch["x"])
        assert PR.expected_h_pub(w.k, BF, A, Lk, prover.CHUNK, ev, ch["beta"], ch["gamma"], ch["y"], ch["x"], prover.DELTA, inst_x) == ev["h"][0][0]
        xn = pow(ch["x"], w.n, R)
        hc = cref.g1_normalize(cref.msm_g1(cref.fr_ints_to_mont([pow(xn, i, R) for i in range(3)]), pr.commitments["h"]))
        com = dict(pr.commitments)
        com.update(fixed=vk_c["fixed"], sigma=vk_c["sigma"], h=[hc])
        assert PR.query_layout_pub(A, Lk, m, S) == [(list(i), list(mem)) for i, mem in prover.query_layout(A, Lk, m, S)]
        assert V.shplonk_check(cref, PR.query_layout_pub(A, Lk, m, S), prover.rotation_points(w.pk.dom, ch["x"]), com, ev, ch["sh_y"], ch["sh_v"],
                               ch["sh_u"], pr.commitments["w1"][0], pr.commitments["w2"][0], w.s_tox)
    inst = [gathered, gathered]
    assert PV.verify_batch(eng, w.params, vk, proofs, seeds, instances=inst) == (True, [True, True])
    assert PV.verify_proof(eng, w.params, vk, proofs[0], seeds[0], instances=gathered) is True
    assert PV.verify_batch_native(eng, w.params, vk, proofs, seeds, instances=inst) == (True, [True, True])
    wire = [PV.proof_to_bytes(eng, vk, p) for p in proofs]
    assert all(len(b) == PV.proof_size_bytes(vk) for b in wire)
    assert PV.verify_batch_bytes(eng, w.params, vk, wire, seeds, instances=inst) == (True, [True, True])
    back = PV.proof_from_bytes(eng, vk, wire[0])
    assert PV.proof_to_bytes(eng, vk, back) == wire[0]                                          # byte-stable round trip
    # the key file: version 2 with the instance column, and today's bytes without it
    blob = PV.vk_to_bytes(eng, vk)
    vk2 = PV.vk_from_bytes(eng, blob)
    assert blob[4:8] == (2).to_bytes(4, "little") and (vk2.n_instance, vk2.n_public, vk2.m, vk2.n_sets) == (1, len(gathered), m, S)
    assert np.array_equal(vk2.sigma, vk.sigma) and np.array_equal(vk2.fixed, vk.fixed)
    old = PV.VerifyingKey(vk.k, BF, A, Lk, -(-(m - 1) // 2), vk.fixed, vk.sigma[:m - 1])
    assert PV.vk_to_bytes(eng, old)[4:8] == (1).to_bytes(4, "little") and len(PV.vk_to_bytes(eng, old)) == 24 + 32 * (2 * A + Lk + 3)
    assert PV.vk_from_bytes(eng, PV.vk_to_bytes(eng, old)).n_instance == 0


# ------------------------------------------------------------------------------------------------------------------ 8. negatives
@pytest.mark.parametrize("kind", KINDS)
def test_wrong_statements_are_refused(eng, cref, worlds, kind):
    """(a)-(e) on every shape: encrypt and encrypt_uniform, where the instance column is the ONLY member of the last product set, and add,
    where it shares a full pair"""
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV
    from paillier_halo2_amd._lib import PZ_ERR_INVALID, PzError

    w = worlds(kind)
    proofs, seeds, good = w.proofs()
    vk = w.vk
    # a third honest proof, of ANOTHER ciphertext under the same key: add takes another pair (c1, c2); encrypt keeps the message (its bits
    # are the key's shape) and the uniform circuit may keep it, both take another randomness r
    nn, g, x, y, res = w.inp
    if kind == "add":
        x2, y2 = x ^ 0x5a5a, y ^ 0x3c3c
        inp2 = (nn, g, x2, y2, P.paillier_add_native(nn, x2, y2))
    else:
        y2 = y ^ 0x3c3c
        assert 0 < y2 < nn
        inp2 = (nn, g, x, y2, P.paillier_enc_native(nn, g, x, y2))
    cols2 = w.witness(inp2)
    other = w.ns.gather_public(cols2.data_ptr())
    assert other == PR.statement(kind, *inp2, w.bits, w.W) and other != good
    s2 = b"pub-third"
    p2 = prover_native.create_proof(w.key, cols2.data_ptr(), prover.HashTranscript(s2), seed=7, instances=other)
    batch, bseeds = [proofs[0], p2, proofs[1]], [seeds[0], s2, seeds[1]]
    wire = [PV.proof_to_bytes(eng, vk, p) for p in batch]
    verifiers = (lambda inst: PV.verify_batch(eng, w.params, vk, batch, bseeds, instances=inst),
                 lambda inst: PV.verify_batch_native(eng, w.params, vk, batch, bseeds, instances=inst),
                 lambda inst: PV.verify_batch_bytes(eng, w.params, vk, wire, bseeds, instances=inst))
    honest = [good, other, good]
    for v in verifiers:
        assert v(honest) == (True, [True, True, True])
    # (a) one instance limb + 1
    bad = [list(s) for s in honest]
    bad[2][3] += 1
    for v in verifiers:
        assert v(bad) == (False, [True, True, False])
    # (b) an instance >= r
    bad = [list(s) for s in honest]
    bad[0][1] = R + bad[0][1] % 5
    for v in verifiers:
        assert v(bad) == (False, [False, True, True])
    # (c) two proofs of different ciphertexts with their instances swapped
    for v in verifiers:
        assert v([other, good, good]) == (False, [False, False, True])
    # (d) the prover is handed instances that differ from the witness
    lie = list(good)
    lie[-1] ^= 1
    sd = b"pub-lie"
    pl = prover_native.create_proof(w.key, w.witness().data_ptr(), prover.HashTranscript(sd), seed=8, instances=lie)
    assert not pl.h_degree_ok
    assert PV.verify_batch_native(eng, w.params, vk, [pl], [sd], instances=[lie]) == (False, [False])
    assert PV.verify_batch(eng, w.params, vk, [pl], [sd], instances=[lie]) == (False, [False])
    pl2 = prover.create_proof(w.pk, w.witness(), prover.HashTranscript(sd), seed=8, tile=8, instances=lie)
    assert not pl2.h_degree_ok and PV.verify_batch_native(eng, w.params, vk, [pl2], [sd], instances=[lie]) == (False, [False])
    # (e) an old entry point on an instance key, or a wrong L: PZ_ERR_INVALID
    h = PV.native_key(eng, w.params, vk)
    try:
        words = np.stack([PV.pack_proof(vk, p.commitments, p.evals) for p in batch])
        for call in (lambda: eng.verify_batch_dev(h, words, bseeds),
                     lambda: eng.verify_batch_dev(h, words, bseeds, instances=[s[:-1] for s in honest]),
                     lambda: eng.verify_batch_bytes_dev(h, np.frombuffer(b"".join(wire), dtype=np.uint8), bseeds),
                     lambda: eng.verify_batch_bytes_dev(h, np.frombuffer(b"".join(wire), dtype=np.uint8), bseeds, instances=[s + [0] for s in honest]),
                     lambda: prover_native.create_proof(w.key, w.witness().data_ptr(), prover.HashTranscript(b"x"), seed=1),
                     lambda: prover_native.create_proof(w.key, w.witness().data_ptr(), prover.HashTranscript(b"x"), seed=1, instances=good[:-1]),
                     lambda: prover_native.create_proof(w.key, w.witness().data_ptr(), prover.HashTranscript(b"x"), seed=1, instances=[R] + good[1:])):
            with pytest.raises(PzError) as ei:
                call()
            assert ei.value.status == PZ_ERR_INVALID
    finally:
        h.free()
    with pytest.raises(ValueError):
        PV.verify_batch_native(eng, w.params, vk, batch, bseeds)
    # the gather refuses a column stride that is no multiple of an element's 4 words
    outw = np.zeros((w.ns.n_public, 4), dtype=np.uint64)
    assert eng.L.pz_public_gather_dev(eng.ctx, C.c_void_p(cols2.data_ptr()), (4 << w.k) + 2, C.c_void_p(w.ns.d_cell_col), C.c_void_p(w.ns.d_cell_row),
                                      w.ns.n_public, C.c_void_p(outw.ctypes.data)) == PZ_ERR_INVALID
    # the key still serves an honest proof after the refused calls
    ok = prover_native.create_proof(w.key, w.witness().data_ptr(), prover.HashTranscript(b"again"), seed=2, instances=good)
    assert ok.h_degree_ok and PV.verify_batch_native(eng, w.params, vk, [ok], [b"again"], instances=[good]) == (True, [True])
