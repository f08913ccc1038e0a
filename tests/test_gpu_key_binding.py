"""GPU: the verifying key's digest bound into the Fiat-Shamir transcript (include/pz.h "KEY BINDING": pz_key_digest, pz_pk_digest,
pz_vk_digest, pz_vk_bind, pz_vk_is_bound; host/key_digest.hpp; prover.key_digest, HashTranscript(seed, key_digest=), bind_key= on the
verifiers; PZ_PROVE_BIND / PZ_VERIFY_BIND of the compiled drivers).  Shapes: add 128 / 64 / k 12 (with and without
the instance column) and encrypt 128 / 64 / k 14, the shapes of tests/test_gpu_public_inputs.py and tests/test_gpu_wire.py.  The replay is
the unmodified oracle's (oracle/verifier.py::replay_challenges) handed digest + seed for its seed bytes.  Every comparison is exact."""
import ctypes as C
import hashlib
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from oracle import pyref as P
from oracle import verifier as V
from tests import public_ref as PR

pytestmark = pytest.mark.gpu

R = P.FR_R
BF = 6
BITS, W = 128, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def ref_digest(k, bf, n_adv, n_lk, n_instance, n_public, fixed, sigma) -> bytes:
    """the definition, written out with hashlib"""
    h = hashlib.blake2b(digest_size=64, person=b"PZ-Key-Digest-v1")
    h.update(struct.pack("<6Q", k, bf, n_adv, n_lk, n_instance, n_public))
    for arr in (fixed, sigma):
        h.update(b"".join(struct.pack("<Q", int(w)) for w in np.asarray(arr, dtype=np.uint64).reshape(-1)))
    return h.digest()


def lib_key_digest(eng, k, bf, n_adv, n_lk, n_instance, n_public, fixed, sigma) -> bytes:
    out = (C.c_uint8 * 64)()
    f, s = np.ascontiguousarray(fixed, dtype=np.uint64), np.ascontiguousarray(sigma, dtype=np.uint64)
    assert eng.L.pz_key_digest(k, bf, n_adv, n_lk, n_instance, n_public, f.ctypes.data, s.ctypes.data, out) == 0
    return bytes(out)


class Srs:
    """ParamsKZG::setup from a known scalar for one k"""

    def __init__(self, eng, cref, k):
        import torch

        from paillier_halo2_amd import srs
        from paillier_halo2_amd import verifier as PV

        self.k, n = k, 1 << k
        self.s_tox = random.Random(0xb1d + k).randrange(2, R)
        F = lambda v: cref.fr_ints_to_mont([v % R])[0]
        self.d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        self.d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(k, F(self.s_tox), F(P.fr_omega(k)), self.d_g.data_ptr(), self.d_gl.data_ptr())
        eng.sync()
        self.g2, self.s_g2 = srs.setup_g2(eng, F(self.s_tox))
        self.params = PV.VerifierParams.from_parts(self.d_g[0].cpu().numpy().view(np.uint64), self.g2, self.s_g2)
        self.bl, self.bm = eng.load_bases_dev(self.d_gl.data_ptr(), n), eng.load_bases_dev(self.d_g.data_ptr(), n)

    def write(self, path):
        from paillier_halo2_amd import srs

        srs.write_params_kzg(path, self.k, self.d_g.cpu().numpy().view(np.uint64), self.d_gl.cpu().numpy().view(np.uint64), self.g2, self.s_g2)

    def close(self):
        self.bl.free()
        self.bm.free()


def witness(eng, cref, kind, ns, inp, lb):
    """the K4 columns [ns.m][2^k][4] of the circuit for inputs (n, g, x, y, res) (tests/test_gpu_public_inputs.py's recipe)"""
    import torch

    nn, g, x, y, res = inp
    Ln, n = BITS // W, 1 << ns.k
    L = 2 * Ln
    arr = lambda v, l: cref.int_to_limbs(v, l)
    if kind == "add":
        q, rem = eng.mul_mod(L, arr(x, L), arr(y, L), arr(nn * nn, L))
        assert cref.limbs_to_int(rem) == res
        d_steps = torch.from_numpy(np.stack([arr(x, L), arr(y, L), q, rem]).astype(np.int64)).cuda().view(1, 4, L)
    else:
        cap = ns.n_steps_g + ns.n_steps_r + 1
        d_steps = torch.zeros((cap, 4, L), dtype=torch.int64, device="cuda")
        c, _, _ = eng.paillier_encrypt_dev(Ln, arr(nn, Ln), arr(g, Ln), arr(x, Ln), arr(y, Ln), d_steps.data_ptr(), cap)
        assert cref.limbs_to_int(c[0]) == res
    d_mod = torch.from_numpy(arr(nn * nn, L).astype(np.int64)).cuda()
    cols = torch.zeros((ns.m, n, 4), dtype=torch.int64, device="cuda")
    inputs = np.concatenate([arr(nn, Ln), arr(g, Ln), arr(x, Ln), arr(y, Ln), arr(res, L)])
    eng.circuit_expand_cols_dev(PR.KIND_ID[kind], Ln, W, lb, inputs, d_steps.data_ptr(), ns.n_steps_g, ns.n_steps_r, d_mod.data_ptr(),
                                cols.data_ptr(), cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, n)
    eng.sync()
    return cols


@pytest.fixture(scope="module")
def add(eng, cref):
    """add, k = 12: the plain structure with both proving keys (the stepper's and prover.py's), the exposed structure with the stepper's"""
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    K, LB = 12, 11
    s = Srs(eng, cref, K)
    inp = PR.inputs("add", BITS, 0x99)
    nn, g, x, y, res = inp
    ns = prover_native.NativeStructure(eng, "add", BITS, W, LB, K, exp_g=x, exp_r=nn)
    ns_pub = prover_native.NativeStructure(eng, "add", BITS, W, LB, K, exp_g=x, exp_r=nn, expose=True)
    key, key_pub = ns.key(s.bl, s.bm, tile=8), ns_pub.key(s.bl, s.bm, tile=8)
    cs, _ = CS.columns(CS.stream_structure("add", BITS, W, LB, x, nn), K, LB, device="cpu")
    pk = prover.keygen(eng, cs, s.bl, s.bm)
    w = dict(K=K, LB=LB, srs=s, inp=inp, ns=ns, ns_pub=ns_pub, key=key, key_pub=key_pub, pk=pk, vk=PV.VerifyingKey.from_proving_key(pk),
             wit=lambda st_, i=None: witness(eng, cref, "add", st_, i or inp, LB))
    yield w
    key.free()
    key_pub.free()
    ns.free()
    ns_pub.free()
    s.close()


def _same_popcount_neighbour(m: int) -> int:
    """another message with m's bit length and popcount: one set and one clear bit below the top bit change places"""
    bits = m.bit_length()
    lo1 = next(i for i in range(bits - 1) if m >> i & 1)
    lo0 = next(i for i in range(bits - 1) if not m >> i & 1)
    m2 = m ^ (1 << lo1) ^ (1 << lo0)
    assert m2 != m and m2.bit_length() == bits and bin(m2).count("1") == bin(m).count("1")
    return m2


@pytest.fixture(scope="module")
def enc(eng, cref):
    """encrypt, k = 14: key K1 of message m with its proving key, and the structure of a second message of the same shape (key K2)"""
    from paillier_halo2_amd import prover_native

    K, LB = 14, 13
    s = Srs(eng, cref, K)
    inp = PR.inputs("encrypt", BITS, 0x50)
    nn, g, m, r, res = inp
    m2 = _same_popcount_neighbour(m)
    ns = prover_native.NativeStructure(eng, "encrypt", BITS, W, LB, K, exp_g=m, exp_r=nn)
    ns2 = prover_native.NativeStructure(eng, "encrypt", BITS, W, LB, K, exp_g=m2, exp_r=nn)
    key = ns.key(s.bl, s.bm)
    w = dict(K=K, LB=LB, srs=s, inp=inp, m2=m2, ns=ns, ns2=ns2, key=key)
    yield w
    key.free()
    ns.free()
    ns2.free()
    s.close()


def _vk_of(key, ns):
    from paillier_halo2_amd import verifier as PV

    c = key.vk_commitments()
    return PV.VerifyingKey(ns.k, BF, ns.n_adv, ns.n_lk, -(-ns.m // 2), c["fixed"], c["sigma"], ns.n_instance, ns.n_public)


# ---- 1. one key, every route, one digest ------------------------------------------------------------------------------------------------
def _routes(eng, s, ns, key, tile):
    from paillier_halo2_amd import verifier as PV

    vk = _vk_of(key, ns)
    shape = (ns.k, BF, ns.n_adv, ns.n_lk, ns.n_instance, ns.n_public)
    want = ref_digest(*shape, vk.fixed, vk.sigma)
    got = {"pz_pk_digest": key.digest()}
    h = PV.native_key(eng, s.params, vk)                                     # pz_vk_create[_pub] from the pk's commitments
    try:
        got["pz_vk_digest"] = h.digest()
        assert h.digest() == got["pz_vk_digest"]                             # the cached one
    finally:
        h.free()
    fx, sg = eng.vk_keygen_dev(s.bl, ns.k, ns.lookup_bits, ns.n_adv, ns.n_lk, ns.d_selectors, ns.constants(), ns.d_map_col, ns.d_map_row, tile,
                               ns.n_instance, ns.n_public)
    got["pz_key_digest(pz_vk_keygen_dev)"] = lib_key_digest(eng, *shape, fx, sg)
    got["from_structure"] = PV.VerifyingKey.from_structure(eng, ns, s.bl, tile=tile).digest()
    got["file round trip"] = PV.vk_from_bytes(eng, PV.vk_to_bytes(eng, vk)).digest()
    got["VerifyingKey.digest"] = vk.digest()
    for name, d in got.items():
        assert d == want, name
    return want


def test_one_key_every_route_one_digest_add(eng, add):
    want = _routes(eng, add["srs"], add["ns"], add["key"], 8)
    assert add["pk"].digest() == add["vk"].digest() == want                  # prover.py's key on the Python structure
    # the exposed key is another key (test 4 uses it)
    assert _routes(eng, add["srs"], add["ns_pub"], add["key_pub"], 8) != want


def test_one_key_every_route_one_digest_encrypt(eng, enc):
    _routes(eng, enc["srs"], enc["ns"], enc["key"], 64)


# ---- 2. bound proofs verify only as bound -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def add_proofs(eng, add):
    """[bound by prover.py, bound by the stepper, unbound by the stepper] with their transcripts and seeds"""
    from paillier_halo2_amd import prover, prover_native

    D = add["key"].digest()
    seeds = [b"bind-python", b"bind-stepper", b"plain-stepper"]
    trs = [prover.HashTranscript(seeds[0], key_digest=add["pk"].digest()), prover.HashTranscript(seeds[1], key_digest=D), prover.HashTranscript(seeds[2])]
    proofs = [prover.create_proof(add["pk"], add["wit"](add["ns"]), trs[0], seed=21, tile=8),
              prover_native.create_proof(add["key"], add["wit"](add["ns"]).data_ptr(), trs[1], seed=22),
              prover_native.create_proof(add["key"], add["wit"](add["ns"]).data_ptr(), trs[2], seed=23)]
    assert all(p.h_degree_ok for p in proofs)
    return dict(D=D, proofs=proofs, trs=trs, seeds=seeds)


def test_bound_proofs_replay_from_digest_then_seed(add, add_proofs):
    D = add_proofs["D"]
    for pr, tr, seed in list(zip(add_proofs["proofs"], add_proofs["trs"], add_proofs["seeds"]))[:2]:
        recorded = dict(tr.drawn)
        assert set(recorded) == {"theta", "beta", "gamma", "y", "x", "sh_y", "sh_v", "sh_u"}
        assert V.replay_challenges(D + seed, pr.commitments, pr.evals) == recorded
        plain = V.replay_challenges(seed, pr.commitments, pr.evals)
        assert all(plain[nm] != recorded[nm] for nm in recorded)
        ch = tr.challenges()
        assert ch.transcript_seed == seed and ch.theta == recorded["theta"]          # the caller's seed, not digest + seed
    pr, tr, seed = add_proofs["proofs"][2], add_proofs["trs"][2], add_proofs["seeds"][2]
    assert V.replay_challenges(seed, pr.commitments, pr.evals) == dict(tr.drawn)      # unbound: as it always was


def test_bound_proofs_verify_only_as_bound(eng, add, add_proofs):
    from paillier_halo2_amd import verifier as PV

    vk, params = add["vk"], add["srs"].params
    proofs, seeds = add_proofs["proofs"], add_proofs["seeds"]
    handle = PV.native_key(eng, params, vk)
    try:
        wire = [PV.proof_to_bytes(eng, vk, p, handle=handle) for p in proofs]
        for i in (0, 1):
            for bind, want in ((True, True), (False, False)):
                assert PV.verify_proof(eng, params, vk, proofs[i], seeds[i], bind_key=bind) is want, (i, bind)
                assert PV.verify_batch(eng, params, vk, [proofs[i]], [seeds[i]], bind_key=bind) == (want, [want]), (i, bind)
                assert PV.verify_batch_native(eng, params, vk, [proofs[i]], [seeds[i]], bind_key=bind) == (want, [want]), (i, bind)
                assert PV.verify_batch_bytes(eng, params, vk, [wire[i]], [seeds[i]], bind_key=bind) == (want, [want]), (i, bind)
                assert PV.verify_batch_native(eng, params, vk, [proofs[i]], [seeds[i]], handle=handle, bind_key=bind) == (want, [want]), (i, bind)
                assert handle.bound is False                                           # a caller's handle gets its own setting back
        # an unbound proof: True as it always was, False under binding
        for bind, want in ((False, True), (True, False)):
            assert PV.verify_proof(eng, params, vk, proofs[2], seeds[2], bind_key=bind) is want
            assert PV.verify_batch_native(eng, params, vk, [proofs[2]], [seeds[2]], bind_key=bind) == (want, [want])
            assert PV.verify_batch_bytes(eng, params, vk, [wire[2]], [seeds[2]], bind_key=bind) == (want, [want])
        # gluing the digest to the seed by hand is the same thing: an unbound verifier handed digest + seed accepts the bound proof
        D = add_proofs["D"]
        assert PV.verify_batch_native(eng, params, vk, proofs[:2], [D + s for s in seeds[:2]]) == (True, [True, True])
        # a mixed batch, binding on
        batch, bseeds, bwire = [proofs[0], proofs[2], proofs[1]], [seeds[0], seeds[2], seeds[1]], [wire[0], wire[2], wire[1]]
        assert PV.verify_batch(eng, params, vk, batch, bseeds, bind_key=True) == (False, [True, False, True])
        assert PV.verify_batch_native(eng, params, vk, batch, bseeds, bind_key=True) == (False, [True, False, True])
        assert PV.verify_batch_bytes(eng, params, vk, bwire, bseeds, bind_key=True) == (False, [True, False, True])
        # ... and off: the complement
        assert PV.verify_batch_native(eng, params, vk, batch, bseeds) == (False, [False, True, False])
        assert PV.verify_batch_bytes(eng, params, vk, bwire, bseeds, handle=handle) == (False, [False, True, False])
    finally:
        handle.free()


# ---- 3. two keys of one shape -------------------------------------------------------------------------------------------------------------
def test_two_keys_of_one_shape(eng, cref, enc):
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    ns, ns2, key, s = enc["ns"], enc["ns2"], enc["key"], enc["srs"]
    assert (ns.n_adv, ns.n_lk, ns.m, ns.max_rows) == (ns2.n_adv, ns2.n_lk, ns2.m, ns2.max_rows)
    assert (ns.n_steps_g, ns.n_steps_r) == (ns2.n_steps_g, ns2.n_steps_r)
    vk1 = _vk_of(key, ns)
    vk2 = PV.VerifyingKey.from_structure(eng, ns2, s.bl)
    D1, D2 = key.digest(), vk2.digest()
    assert vk1.digest() == D1 and D1 != D2
    assert not np.array_equal(vk1.sigma, vk2.sigma) or not np.array_equal(vk1.fixed, vk2.fixed)
    seed = b"two-keys"
    tr = prover.HashTranscript(seed, key_digest=D1)
    pr = prover_native.create_proof(key, witness(eng, cref, "encrypt", ns, enc["inp"], enc["LB"]).data_ptr(), tr, seed=31)
    assert pr.h_degree_ok
    under1, under2 = V.replay_challenges(D1 + seed, pr.commitments, pr.evals), V.replay_challenges(D2 + seed, pr.commitments, pr.evals)
    assert under1 == dict(tr.drawn) and under1["theta"] != under2["theta"]
    assert PV.verify_batch_native(eng, s.params, vk1, [pr], [seed], bind_key=True) == (True, [True])
    assert PV.verify_batch_native(eng, s.params, vk2, [pr], [seed], bind_key=True) == (False, [False])
    assert PV.verify_batch(eng, s.params, vk2, [pr], [seed], bind_key=True) == (False, [False])
    assert PV.verify_batch_bytes(eng, s.params, vk2, [PV.proof_to_bytes(eng, vk1, pr)], [seed], bind_key=True) == (False, [False])


# ---- 4. with the instance column --------------------------------------------------------------------------------------------------------
def test_bound_and_stated_proofs(eng, add):
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    ns, key, params = add["ns_pub"], add["key_pub"], add["srs"].params
    vk = _vk_of(key, ns)
    assert (vk.n_instance, vk.n_public) == (1, ns.n_public) and ns.n_public > 0
    D = key.digest()
    assert D == vk.digest() != add["key"].digest()
    # the column alone moves the digest: the unexposed key's arrays are not a prefix that hashes the same
    cols = add["wit"](ns)
    stated = ns.gather_public(cols.data_ptr())
    seed = b"bound-and-stated"
    tr = prover.HashTranscript(seed, key_digest=D)
    pr = prover_native.create_proof(key, cols.data_ptr(), tr, seed=41, instances=stated)
    assert pr.h_degree_ok
    assert PR.replay_challenges_pub(D + seed, stated, pr.commitments, pr.evals) == dict(tr.drawn)
    wire = PV.proof_to_bytes(eng, vk, pr)
    for bind, want in ((True, True), (False, False)):
        assert PV.verify_batch_native(eng, params, vk, [pr], [seed], instances=[stated], bind_key=bind) == (want, [want])       # pz_verify_batch_pub
        assert PV.verify_batch_bytes(eng, params, vk, [wire], [seed], instances=[stated], bind_key=bind) == (want, [want])      # pz_verify_batch_bytes_pub
        assert PV.verify_batch(eng, params, vk, [pr], [seed], instances=[stated], bind_key=bind) == (want, [want])
    lie = list(stated)
    lie[0] ^= 1
    assert PV.verify_batch_native(eng, params, vk, [pr], [seed], instances=[lie], bind_key=True) == (False, [False])


# ---- 5. the compiled drivers ----------------------------------------------------------------------------------------------------------------
def _gxx(src, exe):
    csrc = os.path.join(ROOT, "paillier_halo2_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe, os.path.join(ROOT, "paillier_halo2_amd", "host", src),
                    "-L" + csrc, "-lpz_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def _env(**kw):
    e = {k: v for k, v in os.environ.items() if k not in ("PZ_PROVE_BIND", "PZ_VERIFY_BIND", "PZ_PROVE_WIRE", "PZ_PROVE_VIA_STEPPER")}
    e.update(kw)
    return e


@pytest.fixture(scope="module")
def drivers(eng, cref, enc, tmp_path_factory):
    """tests/test_gpu_wire.py's job (encrypt 128 / 64 / k 14, two proofs, tile 64) proved four times: unbound twice, bound, bound through the
    stepper; the two verifiers compiled"""
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import prover_job

    d = tmp_path_factory.mktemp("bind")
    nn, g, m, r, _ = enc["inp"]
    sa = CS.stream_structure("encrypt", BITS, W, enc["LB"], m, nn)
    st, starts = CS.columns(sa, enc["K"], enc["LB"], device="cpu")
    job, params = str(d / "job.bin"), str(d / "kzg_bn254_14.srs")
    enc["srs"].write(params)
    prover_job.write_job(job, st, starts, BITS, 0, sa.n_steps_g, sa.n_steps_r, nn, g, [(m, r), (m, random.Random(0x6a6f64).randrange(1, nn))],
                         enc["srs"].s_tox, seed=7, proofs=2, tile=64)
    runs = {}
    for name, env in (("plain_a", _env(PZ_PROVE_WIRE="1")), ("plain_b", _env(PZ_PROVE_WIRE="1")), ("bound", _env(PZ_PROVE_WIRE="1", PZ_PROVE_BIND="1")),
                      ("bound_stepper", _env(PZ_PROVE_WIRE="1", PZ_PROVE_BIND="1", PZ_PROVE_VIA_STEPPER="1"))):
        out = str(d / (name + ".bin"))
        line = prover_job.run(job, out, env=env)
        assert line["quotient_degree_ok"] is True and line["proofs"] == 2, name
        runs[name] = out
    exes = {}
    for src in ("verify_wire", "verify_connected", "keygen_vk"):
        exes[src] = str(d / src)
        _gxx(src + ".cpp", exes[src])
    return dict(job=job, params=params, runs=runs, exes=exes, st=st, dir=d)


def _files(proof):
    return [proof, proof + ".vk", proof + ".p0.bin", proof + ".p1.bin"]


def test_unbound_runs_are_byte_identical_and_a_bound_run_is_not(drivers):
    a, b, c = (_files(drivers["runs"][nm]) for nm in ("plain_a", "plain_b", "bound"))
    rd = lambda p: open(p, "rb").read()
    for fa, fb in zip(a, b):
        assert rd(fa) == rd(fb), fa
    assert rd(a[1]) == rd(c[1])                                  # the key file does not change: the digest is computable from what it holds
    for fa, fc in ((a[0], c[0]), (a[2], c[2]), (a[3], c[3])):
        assert len(rd(fa)) == len(rd(fc)) and rd(fa) != rd(fc), fa


def test_compiled_bound_proofs_replay_from_the_keys_digest(enc, drivers):
    from paillier_halo2_amd import consts, prover_job
    from paillier_halo2_amd import verifier as PV

    D = enc["key"].digest()
    st = drivers["st"]
    for name, bound in (("plain_a", False), ("bound", True), ("bound_stepper", True)):
        rec = prover_job.read_proofs(drivers["runs"][name])
        vk = PV.VerifyingKey(st.k, st.blinding_factors, st.n_adv, st.n_lk, -(-st.m // 2), rec["vk/fixed"], rec["vk/sigma"])
        assert vk.digest() == D, name                            # the job's key is the shape's key: pz_pk_digest of the library's own structure
        for i in range(2):
            com, ev = PV.proof_from_record(rec, "p%d/" % i, vk)
            seed = i.to_bytes(8, "little")
            ch = V.replay_challenges((D if bound else b"") + seed, com, ev)
            for nm, v in ch.items():
                assert consts.limbs_to_int(rec["p%d/ch/%s" % (i, nm)][0]) == v, (name, i, nm)
            other = V.replay_challenges((b"" if bound else D) + seed, com, ev)
            assert other["theta"] != ch["theta"]


@pytest.mark.parametrize("verifier", ("verify_wire", "verify_connected"))
def test_compiled_verifiers_accept_bound_proofs_only_when_bound(drivers, verifier):
    exe = drivers["exes"][verifier]

    def run(proof, **env):
        args = [proof + ".vk", drivers["params"], proof + ".p0.bin", proof + ".p1.bin"] if verifier == "verify_wire" else \
            [drivers["job"], drivers["params"], proof]
        r_ = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=_env(**env))
        assert r_.returncode in (0, 1), r_.stderr
        out = json.loads(r_.stdout.strip().splitlines()[-1])
        assert out["proofs"] == 2 and out["verified"] is (r_.returncode == 0) and out["per_proof"] == [r_.returncode == 0] * 2
        return r_.returncode

    runs = drivers["runs"]
    assert run(runs["bound"], PZ_VERIFY_BIND="1") == 0
    assert run(runs["bound"]) == 1
    assert run(runs["bound_stepper"], PZ_VERIFY_BIND="1") == 0
    assert run(runs["plain_a"]) == 0
    assert run(runs["plain_a"], PZ_VERIFY_BIND="1") == 1
    assert run(runs["plain_a"], PZ_VERIFY_BIND="0") == 0                                     # only "1" turns it on


def test_keygen_vk_prints_the_keys_digest(enc, drivers):
    from paillier_halo2_amd import layout

    nn, g, m, r, _ = enc["inp"]
    out = str(drivers["dir"] / "derived.vk")
    r_ = subprocess.run([drivers["exes"]["keygen_vk"], drivers["params"], "encrypt", str(BITS), str(W), str(enc["LB"]), str(enc["K"]),
                         str(layout.MINIMUM_ROWS_BENCH), str(BF), "%x" % m, "%x" % nn, out], capture_output=True, text=True, timeout=300)
    assert r_.returncode == 0, r_.stderr
    info = json.loads(r_.stdout.strip().splitlines()[-1])
    assert info["digest"] == enc["key"].digest().hex() and len(info["digest"]) == 128
    assert open(out, "rb").read() == open(drivers["runs"]["bound"] + ".vk", "rb").read()


def test_fresh_mode_binds_each_step_to_its_own_key(enc, tmp_path):
    from paillier_halo2_amd import consts, prover_job
    from paillier_halo2_amd import verifier as PV

    nn, g, m, r, _ = enc["inp"]
    params, out = str(tmp_path / "fresh.bin"), str(tmp_path / "fresh_proofs.bin")
    prover_job.write_fresh_params(params, BITS, enc["K"], enc["LB"], [(nn, g, m, r), (nn, g, enc["m2"], r)], enc["srs"].s_tox, seed=3, tile=64)
    line = prover_job.run_fresh(params, out, env=_env(PZ_PROVE_BIND="1", PZ_PROVE_ARENA_GB="2"))     # (a small arena: these keys are < 1 GB)
    assert line["quotient_degree_ok"] is True and line["steps"] == 2
    rec = prover_job.read_proofs(out)
    digests = []
    for i in range(2):
        pre = "p%d/" % i
        A, Lk, m_cols, S = (int(v) for v in rec[pre + "shape"][0][:4])
        vk = PV.VerifyingKey(enc["K"], BF, A, Lk, S, rec[pre + "vk/fixed"], rec[pre + "vk/sigma"])
        D = vk.digest()
        digests.append(D)
        com, ev = PV.proof_from_record(rec, pre, vk)
        ch = V.replay_challenges(D + i.to_bytes(8, "little"), com, ev)
        for nm, v in ch.items():
            assert consts.limbs_to_int(rec[pre + "ch/" + nm][0]) == v, (i, nm)
    assert digests[0] == enc["key"].digest() and digests[0] != digests[1]                   # step 0's key is K1, step 1's the second message's


# ---- 6. pz_vk_bind / pz_vk_is_bound -------------------------------------------------------------------------------------------------------
def test_bind_round_trip_and_null_keys(eng, add):
    from paillier_halo2_amd import verifier as PV
    from paillier_halo2_amd._lib import PZ_ERR_INVALID, PZ_OK

    L = eng.L
    h = PV.native_key(eng, add["srs"].params, add["vk"])
    try:
        on = C.c_int(-1)
        assert L.pz_vk_is_bound(h.handle, C.byref(on)) == PZ_OK and on.value == 0           # default off
        for setting, want in ((1, 1), (0, 0), (5, 1), (1, 1), (0, 0)):
            assert L.pz_vk_bind(h.handle, setting) == PZ_OK
            assert L.pz_vk_is_bound(h.handle, C.byref(on)) == PZ_OK and on.value == want
            assert h.bound is bool(want)
        h.bind()
        assert h.bound is True
        h.bind(False)
        assert L.pz_vk_is_bound(h.handle, None) == PZ_ERR_INVALID
        out = (C.c_uint8 * 64)()
        assert L.pz_vk_digest(h.handle, None) == PZ_ERR_INVALID and L.pz_pk_digest(add["key"].handle, None) == PZ_ERR_INVALID
        assert L.pz_vk_digest(h.handle, out) == PZ_OK and bytes(out) == add["vk"].digest()
    finally:
        h.free()
    out = (C.c_uint8 * 64)()
    assert L.pz_vk_bind(None, 1) == PZ_ERR_INVALID and L.pz_vk_is_bound(None, C.byref(on)) == PZ_ERR_INVALID
    assert L.pz_vk_digest(None, out) == PZ_ERR_INVALID and L.pz_pk_digest(None, out) == PZ_ERR_INVALID
