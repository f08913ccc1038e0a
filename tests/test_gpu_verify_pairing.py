"""GPU: the product verifier (paillier_halo2_amd/verifier.py) checks proofs of the reference's bench shape (128-bit n, 64-bit limbs,
k = 14, lookup_bits 13) through the pairing on the device, from g[0], g2 and s_g2 alone -- it never sees the toxic scalar -- and agrees
with the oracle's s-collapsed verdict (oracle/verifier.py) on honest and tampered proofs."""
import random
import time

import numpy as np
import pytest

from oracle import pyref as P
from oracle import verifier as V

pytestmark = pytest.mark.gpu

K, LB, BITS, W = 14, 13, 128, 64
R = P.FR_R
N_PROOFS = 8


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

    rng = random.Random(0x7061)
    s_tox = rng.randrange(2, R)
    F = lambda v: cref.fr_ints_to_mont([v % R])[0]
    d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    eng.srs_setup_g1_dev(K, F(s_tox), F(consts.fr_omega(K)), d_g.data_ptr(), d_gl.data_ptr())
    eng.sync()
    # the verifier's params: g[0], g2, s_g2 through a params file (the scalar s stays here)
    g2, s_g2 = srs.setup_g2(eng, F(s_tox))
    path = str(tmp_path_factory.mktemp("params") / "kzg_bn254_14.srs")
    srs.write_params_kzg(path, K, d_g.cpu().numpy().view(np.uint64), d_gl.cpu().numpy().view(np.uint64), g2, s_g2)
    params = srs.read_params_kzg(path, K)
    vparams = PV.VerifierParams.from_params(params)
    bl, bm = eng.load_bases_dev(d_gl.data_ptr(), n), eng.load_bases_dev(d_g.data_ptr(), n)
    pk = prover.keygen(eng, st, bl, bm)
    vk = PV.VerifyingKey.from_proving_key(pk)
    proofs, seeds = [], []
    for i in range(N_PROOFS):
        seed = b"verify-%d" % i
        tr = prover.HashTranscript(seed)
        proofs.append(prover.create_proof(pk, witness(), tr, seed=100 + i, tile=64))
        seeds.append(seed)
    yield dict(st=st, starts=starts, pk=pk, vk=vk, params=vparams, params_path=path, proofs=proofs, seeds=seeds, s_tox=s_tox,
               inputs=(nn, g, m, r, ng, nr), d_g=d_g)
    bl.free()
    bm.free()


def _oracle_verdict(cref, world, com, ev_words, seed, vk):
    """the oracle's check with the known s: replayed challenges, expected_h, shplonk_check"""
    from paillier_halo2_amd import prover

    st = world["st"]
    A, Lk, m = st.n_adv, st.n_lk, st.m
    S = -(-m // prover.CHUNK)
    ch = V.replay_challenges(seed, com, ev_words)

    def ints(a):
        a = np.asarray(a, dtype=np.uint64)
        flat = cref.fr_mont_to_ints(a.reshape(-1, 4))
        p = a.shape[1]
        return [flat[i * p:(i + 1) * p] for i in range(a.shape[0])]

    ev = {k: ints(v) for k, v in ev_words.items()}
    want = V.expected_h(K, st.blinding_factors, A, Lk, prover.CHUNK, ev, ch["beta"], ch["gamma"], ch["y"], ch["x"], prover.DELTA)
    if com["h"].shape != (3, 8):
        return False
    ident = want == ev["h"][0][0]
    xn = pow(ch["x"], 1 << K, R)
    hc = cref.g1_normalize(cref.msm_g1(cref.fr_ints_to_mont([pow(xn, i, R) for i in range(3)]), com["h"]))
    c = dict(com)
    c.update(fixed=vk.fixed, sigma=vk.sigma, h=[hc])
    lay = prover.query_layout(A, Lk, m, S)
    pts = prover.rotation_points(prover.Domain(K, st.blinding_factors), ch["x"])
    opening = V.shplonk_check(cref, lay, pts, c, ev, ch["sh_y"], ch["sh_v"], ch["sh_u"], com["w1"][0], com["w2"][0], world["s_tox"])
    return bool(ident and opening)


def _copy(pr):
    from paillier_halo2_amd import prover

    return prover.Proof(commitments={k: v.copy() for k, v in pr.commitments.items()}, evals={k: v.copy() for k, v in pr.evals.items()})


def test_batch_of_honest_proofs_verifies(eng, cref, world):
    from paillier_halo2_amd import verifier as PV

    ok, per = PV.verify_batch(eng, world["params"], world["vk"], world["proofs"], world["seeds"])
    t0 = time.perf_counter()
    ok2, _ = PV.verify_batch(eng, world["params"], world["vk"], world["proofs"], world["seeds"])
    print("\nverify_batch: %d proofs at k = %d in %.1f ms" % (N_PROOFS, K, (time.perf_counter() - t0) * 1e3))
    assert ok and ok2 and per == [True] * N_PROOFS
    for pr, seed in zip(world["proofs"], world["seeds"]):
        assert _oracle_verdict(cref, world, pr.commitments, pr.evals, seed, world["vk"]) is True
    t0 = time.perf_counter()
    assert PV.verify_proof(eng, world["params"], world["vk"], world["proofs"][0], world["seeds"][0])
    print("verify_proof: 1 proof in %.1f ms" % ((time.perf_counter() - t0) * 1e3))


def test_tampered_proofs_are_rejected(eng, cref, world):
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
        got = PV.verify_proof(eng, world["params"], key, pr, sd)
        want = _oracle_verdict(cref, world, pr.commitments, pr.evals, sd, key)
        assert got is False and want is False, name


def test_batch_flags_exactly_the_tampered_proof(eng, world):
    from paillier_halo2_amd import verifier as PV

    proofs = list(world["proofs"])
    t = _copy(proofs[5])
    t.commitments["w2"] = t.commitments["w1"].copy()
    proofs[5] = t
    ok, per = PV.verify_batch(eng, world["params"], world["vk"], proofs, world["seeds"])
    assert ok is False and per == [i != 5 for i in range(N_PROOFS)]


def test_compiled_prover_records_verify(eng, cref, world, tmp_path):
    from paillier_halo2_amd import prover_job
    from paillier_halo2_amd import verifier as PV

    st, (nn, g, m, r, ng, nr) = world["st"], world["inputs"]
    rng = random.Random(0x6a6f63)
    msgs = [(m, r), (m, rng.randrange(1, nn))]
    job, proof = str(tmp_path / "job.bin"), str(tmp_path / "proof.bin")
    prover_job.write_job(job, st, world["starts"], BITS, 0, ng, nr, nn, g, msgs, world["s_tox"], seed=7, proofs=2, tile=64)
    line = prover_job.run(job, proof)
    assert line["quotient_degree_ok"] is True and line["proofs"] == 2
    rec = prover_job.read_proofs(proof)
    vk = world["vk"]
    rvk = PV.VerifyingKey(K, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.n_sets, rec["vk/fixed"], rec["vk/sigma"])
    items = [(rec, "p0/"), (rec, "p1/")]
    seeds = [PV.record_seed(p) for _, p in items]
    ok, per = PV.verify_batch(eng, world["params"], rvk, items, seeds)
    assert ok and per == [True, True]
    bad = {k: v.copy() for k, v in rec.items()}
    bad["p1/c/w2"] = bad["p1/c/w1"].copy()
    ok, per = PV.verify_batch(eng, world["params"], rvk, [(bad, "p0/"), (bad, "p1/")], seeds)
    assert ok is False and per == [True, False]


def test_zero_g2_params_raise(eng, world, tmp_path):
    from paillier_halo2_amd import srs
    from paillier_halo2_amd import verifier as PV

    p = srs.read_params_kzg(world["params_path"], K)
    path = str(tmp_path / "zero_g2.srs")
    srs.write_params_kzg(path, K, p.g, p.g_lagrange)
    with pytest.raises(ValueError):
        PV.verify_batch(eng, srs.read_params_kzg(path, K), world["vk"], world["proofs"][:1], world["seeds"][:1])
