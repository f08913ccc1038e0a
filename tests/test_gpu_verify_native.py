"""GPU: the device batch verifier (include/pz.h: pz_vk_create / pz_verify_batch; paillier_halo2_amd/verifier.py::verify_batch_native and
host/verify_connected.cpp) at the reference's bench shape (128-bit n, 64-bit limbs, k = 14, lookup_bits 13): the same verdicts as the Python
verifier (verify_batch / verify_proof), h(x) word for word as the Python path implies it, each proof's SHPLONK points A and B as
verifier._terms forms them, and the compiled driver on prove_connected's proof file."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyref as P

pytestmark = pytest.mark.gpu

K, LB, BITS, W = 14, 13, 128, 64
R = P.FR_R
N_PROOFS = 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(eng, cref, tmp_path_factory):
    import torch

    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import consts, prover, srs
    from paillier_halo2_amd import verifier as PV

    nn, g, m, r = P.synth_paillier_inputs(BITS, 0x5042, standard_g=False)
    res = P.paillier_enc_native(nn, g, m, r)
    sa = CS.stream_structure("encrypt", BITS, W, LB, m, nn)
    ng, nr = sa.n_steps_g, sa.n_steps_r
    st, starts = CS.columns(sa, K, LB, device="cpu")
    n, Ln = 1 << K, BITS // W
    d_starts = torch.from_numpy(np.asarray(starts, dtype=np.int64)).cuda()
    arr = lambda v, l: cref.int_to_limbs(v, l)

    def witness():
        cap = ng + nr + 1
        d_steps = torch.zeros((cap, 4, 2 * Ln), dtype=torch.int64, device="cuda")
        eng.paillier_encrypt_dev(Ln, arr(nn, Ln), arr(g, Ln), arr(m, Ln), arr(r, Ln), d_steps.data_ptr(), cap)
        d_mod = torch.from_numpy(arr(nn * nn, 2 * Ln).astype(np.int64)).cuda()
        cols = torch.zeros((st.m, n, 4), dtype=torch.int64, device="cuda")
        inputs = np.concatenate([arr(nn, Ln), arr(g, Ln), arr(m, Ln), arr(r, Ln), arr(res, 2 * Ln)])
        eng.circuit_expand_cols_dev(0, Ln, W, LB, inputs, d_steps.data_ptr(), ng, nr, d_mod.data_ptr(), cols.data_ptr(),
                                    cols[st.n_adv].data_ptr(), d_starts.data_ptr(), st.n_adv, st.max_rows, st.max_rows, n)
        eng.sync()
        return cols

    rng = random.Random(0x7662)
    s_tox = rng.randrange(2, R)
    F = lambda v: cref.fr_ints_to_mont([v % R])[0]
    d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    eng.srs_setup_g1_dev(K, F(s_tox), F(consts.fr_omega(K)), d_g.data_ptr(), d_gl.data_ptr())
    eng.sync()
    g2, s_g2 = srs.setup_g2(eng, F(s_tox))
    path = str(tmp_path_factory.mktemp("params") / "kzg_bn254_14.srs")
    srs.write_params_kzg(path, K, d_g.cpu().numpy().view(np.uint64), d_gl.cpu().numpy().view(np.uint64), g2, s_g2)
    vparams = PV.VerifierParams.from_params(srs.read_params_kzg(path, K))
    bl, bm = eng.load_bases_dev(d_gl.data_ptr(), n), eng.load_bases_dev(d_g.data_ptr(), n)
    pk = prover.keygen(eng, st, bl, bm)
    vk = PV.VerifyingKey.from_proving_key(pk)
    proofs, seeds = [], []
    for i in range(N_PROOFS):
        seed = b"native-%d" % i
        proofs.append(prover.create_proof(pk, witness(), prover.HashTranscript(seed), seed=200 + i, tile=64))
        seeds.append(seed)
    yield dict(st=st, starts=starts, vk=vk, params=vparams, params_path=path, proofs=proofs, seeds=seeds, s_tox=s_tox,
               inputs=(nn, g, m, r, ng, nr))
    bl.free()
    bm.free()


def _copy(pr):
    from paillier_halo2_amd import prover

    return prover.Proof(commitments={k: v.copy() for k, v in pr.commitments.items()}, evals={k: v.copy() for k, v in pr.evals.items()})


def _python_h(vk, pr, seed):
    """h(x) as the Python path implies it: the constraint expression at the replayed challenges times (x^n - 1)^-1"""
    from paillier_halo2_amd import verifier as PV

    ch = PV.replay_transcript(seed, pr.commitments, pr.evals)
    e = {f: PV._ints(pr.evals[f]) for f in ("advice", "lookup_advice", "fixed", "sigma", "perm_z", "lookup_z", "perm_inputs", "perm_tables",
                                            "random")}
    x = ch["x"]
    return PV.constraint_expression(vk, e, ch["beta"], ch["gamma"], ch["y"], x) * pow(pow(x, 1 << vk.k, R) - 1, -1, R) % R


def test_honest_batch_h_and_shplonk_points(eng, cref, world):
    from paillier_halo2_amd import consts
    from paillier_halo2_amd import verifier as PV

    vk, params, proofs, seeds = world["vk"], world["params"], world["proofs"], world["seeds"]
    assert PV.verify_batch_native(eng, params, vk, proofs, seeds) == (True, [True] * N_PROOFS)
    h = PV.native_key(eng, params, vk)
    try:
        words = np.stack([PV.pack_proof(vk, p.commitments, p.evals) for p in proofs])
        assert words.shape == (N_PROOFS, h.proof_words)
        ok, per, hev, ab = eng.verify_batch_dev(h, words, seeds, want_h=True, want_ab=True)
    finally:
        h.free()
    assert ok is True and per == [True] * N_PROOFS          # the per-proof path (asked for A and B) agrees
    for i, (pr, sd) in enumerate(zip(proofs, seeds)):
        assert np.array_equal(hev[i], consts.fr_mont_limbs(_python_h(vk, pr, sd))), i
        t = PV._terms(vk, pr.commitments, pr.evals, sd)
        assert t.ok
        bases = np.concatenate([vk.fixed.reshape(-1, 8), vk.sigma.reshape(-1, 8), params.g0.reshape(1, 8), t.bases])
        sa = cref.fr_ints_to_mont([int(v) % R for v in t.vk_scalars] + [t.g_scalar] + [int(v) for v in t.a_scalars])
        sb = cref.fr_ints_to_mont([int(v) for v in t.b_scalars])
        want_a = cref.g1_normalize(cref.msm_g1(sa, bases))
        want_b = cref.g1_normalize(cref.msm_g1(sb, t.bases))
        assert np.array_equal(ab[i, 0], np.asarray(want_a).reshape(8)), i
        assert np.array_equal(ab[i, 1], np.asarray(want_b).reshape(8)), i


def test_tampered_proofs_are_rejected_like_the_python_verifier(eng, cref, world):
    from paillier_halo2_amd import consts
    from paillier_halo2_amd import verifier as PV

    base, seed, vk = world["proofs"][1], world["seeds"][1], world["vk"]
    cases = []
    t = _copy(base)                                       # 1. one evaluation
    v = cref.fr_mont_to_ints(t.evals["advice"][2, 1].reshape(1, 4))[0]
    t.evals["advice"][2, 1] = consts.fr_mont_limbs(v + 1)
    cases.append(("evaluation", t, seed, vk))
    t = _copy(base)                                       # 2. W2 + G
    w2 = cref.affine_mont_to_ints(t.commitments["w2"])[0]
    t.commitments["w2"] = cref.affine_ints_to_mont([P.g1_add_aff(w2, P.G1_GEN)])
    cases.append(("w2", t, seed, vk))
    t = _copy(base)                                       # 3. one advice commitment
    t.commitments["advice"][0] = t.commitments["advice"][1]
    cases.append(("advice commitment", t, seed, vk))
    vk2 = PV.VerifyingKey(vk.k, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.n_sets, vk.fixed, np.roll(vk.sigma, 1, axis=0))
    cases.append(("sigma of another key", base, seed, vk2))   # 4. another copy-constraint map's sigma commitments
    cases.append(("seed", base, b"another seed", vk))     # 5. a wrong transcript seed
    t = _copy(base)                                       # 6. h pieces reordered
    t.commitments["h"] = t.commitments["h"][[1, 0, 2]]
    cases.append(("h order", t, seed, vk))
    for name, pr, sd, key in cases:
        got = PV.verify_batch_native(eng, world["params"], key, [pr], [sd])
        want = PV.verify_proof(eng, world["params"], key, pr, sd)
        assert got == (False, [False]) and want is False, name


def test_batch_flags_exactly_the_tampered_proof(eng, world):
    from paillier_halo2_amd import verifier as PV

    proofs = list(world["proofs"])
    t = _copy(proofs[5])
    t.commitments["w2"] = t.commitments["w1"].copy()
    proofs[5] = t
    ok, per = PV.verify_batch_native(eng, world["params"], world["vk"], proofs, world["seeds"])
    assert ok is False and per == [i != 5 for i in range(N_PROOFS)]


def test_batch_of_one(eng, world):
    from paillier_halo2_amd import verifier as PV

    assert PV.verify_batch_native(eng, world["params"], world["vk"], world["proofs"][3:4], world["seeds"][3:4]) == (True, [True])


def test_vk_create_refuses_zero_g2_and_identity_g0(eng, world):
    import paillier_halo2_amd as pz

    vk, p = world["vk"], world["params"]
    z16 = np.zeros(16, dtype=np.uint64)
    args = (vk.k, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.fixed, vk.sigma)
    for g0, g2, s_g2 in ((p.g0, z16, p.s_g2), (p.g0, p.g2, z16), (np.zeros(8, dtype=np.uint64), p.g2, p.s_g2)):
        with pytest.raises(pz.PzError):
            eng.vk_create(*args, g0, g2, s_g2)
    eng.vk_create(*args, p.g0, p.g2, p.s_g2).free()


@pytest.fixture(scope="module")
def compiled(world, tmp_path_factory):
    """prove_connected's file of two proofs, and the job it came from"""
    from paillier_halo2_amd import prover_job

    st, (nn, g, m, r, ng, nr) = world["st"], world["inputs"]
    d = tmp_path_factory.mktemp("compiled")
    rng = random.Random(0x6a6f64)
    job, proof = str(d / "job.bin"), str(d / "proof.bin")
    prover_job.write_job(job, st, world["starts"], BITS, 0, ng, nr, nn, g, [(m, r), (m, rng.randrange(1, nn))], world["s_tox"], seed=7,
                         proofs=2, tile=64)
    line = prover_job.run(job, proof)
    assert line["quotient_degree_ok"] is True and line["proofs"] == 2
    return job, proof


def test_compiled_prover_records_verify(eng, world, compiled):
    from paillier_halo2_amd import prover_job
    from paillier_halo2_amd import verifier as PV

    rec = prover_job.read_proofs(compiled[1])
    vk = world["vk"]
    rvk = PV.VerifyingKey(K, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.n_sets, rec["vk/fixed"], rec["vk/sigma"])
    seeds = [PV.record_seed("p0/"), PV.record_seed("p1/")]
    assert PV.verify_batch_native(eng, world["params"], rvk, [(rec, "p0/"), (rec, "p1/")], seeds) == (True, [True, True])
    bad = {k: v.copy() for k, v in rec.items()}
    bad["p1/c/w2"] = bad["p1/c/w1"].copy()
    assert PV.verify_batch_native(eng, world["params"], rvk, [(bad, "p0/"), (bad, "p1/")], seeds) == (False, [True, False])


def _record_offset(words, name):
    """word offset of record `name`'s data in a prove_connected proof file"""
    p = 0
    while p < len(words):
        ln = int(words[p])
        nw = (ln + 7) // 8
        nm = words[p + 1:p + 1 + nw].tobytes()[:ln].decode()
        p += 1 + nw
        count, per = int(words[p + 1]), int(words[p + 2])
        p += 3
        if nm == name:
            return p
        p += count * per
    raise KeyError(name)


def test_compiled_driver_verifies_the_proof_file(world, compiled, tmp_path):
    csrc = os.path.join(ROOT, "paillier_halo2_amd", "csrc")
    exe = str(tmp_path / "verify_connected")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-o", exe, os.path.join(ROOT, "paillier_halo2_amd", "host", "verify_connected.cpp"),
                    "-L" + csrc, "-lpz_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    job, proof = compiled
    r = subprocess.run([exe, job, world["params_path"], proof], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    print("\nverify_connected:", line)
    assert line["proofs"] == 2 and line["verified"] is True and line["per_proof"] == [True, True]
    w = np.fromfile(proof, dtype="<u8")
    w[_record_offset(w, "p1/e/advice") + 5] ^= 1          # one word of one evaluation (still below r)
    bad = str(tmp_path / "bad.bin")
    w.tofile(bad)
    r = subprocess.run([exe, job, world["params_path"], bad], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["verified"] is False and line["per_proof"] == [True, False]
    r = subprocess.run([exe, job, world["params_path"], job], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
