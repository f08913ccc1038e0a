"""GPU: halo2 wire bytes on the device (csrc/pz_wire.hip; include/pz.h pz_g1_*compress, pz_proof_encode / decode, pz_verify_batch_bytes;
verifier.proof_to_bytes / proof_from_bytes / verify_batch_bytes; host/verify_wire.cpp) against the Python-integer statement of the format
(tests/wire_ref.py), at the reference's bench shape (128-bit n, 64-bit limbs, k = 14, lookup_bits 13: the world of
tests/test_gpu_verify_native.py, rebuilt here)."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyref as P
from tests import wire_ref as WR

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
        seed = b"wire-%d" % i
        proofs.append(prover.create_proof(pk, witness(), prover.HashTranscript(seed), seed=300 + i, tile=64))
        seeds.append(seed)
    handle = PV.native_key(eng, vparams, vk)
    data = [PV.proof_to_bytes(eng, vk, p, handle=handle) for p in proofs]
    yield dict(st=st, starts=starts, vk=vk, params=vparams, params_path=path, proofs=proofs, seeds=seeds, s_tox=s_tox,
               inputs=(nn, g, m, r, ng, nr), handle=handle, bytes=data)
    handle.free()
    bl.free()
    bm.free()


def _copy(pr):
    from paillier_halo2_amd import prover

    return prover.Proof(commitments={k: v.copy() for k, v in pr.commitments.items()}, evals={k: v.copy() for k, v in pr.evals.items()})


def _off_curve_x(rng):
    while True:
        x = rng.randrange(1, WR.P)
        if WR.decompress(x.to_bytes(32, "little"))[0] == WR.OFF_CURVE:
            return x


# ---- 1. the point codec ----------------------------------------------------------------------------------------------------------------
def test_points_compress_as_the_reference_says_and_come_back(eng, cref):
    rng = random.Random(0x706f696e74)
    sc = cref.fr_ints_to_mont([rng.randrange(1, R) for _ in range(4093)])
    special = np.array([WR.point_words(None), WR.point_words((1, 2)), WR.point_words((1, WR.P - 2))], dtype=np.uint64)
    pts = np.concatenate([eng.g1_fixed_base_mul(sc).reshape(-1, 8), special])
    assert pts.shape == (4096, 8)
    got = eng.g1_compress(pts)
    want = [WR.compress(p) for p in WR.points_from_words(pts)]
    assert [bytes(row) for row in got] == want
    assert want[-3:] == [bytes(32), bytes([1]) + bytes(31), bytes([1]) + bytes(30) + bytes([0x80])]
    back, st = eng.g1_decompress(got)
    assert not st.any() and np.array_equal(back, pts)
    # the device-pointer forms give the same
    d = eng.dev_alloc(4096 * (64 + 32 + 64 + 4))
    try:
        d_pts, d_b, d_back, d_st = d, d + 4096 * 64, d + 4096 * 96, d + 4096 * 160
        eng.upload(d_pts, pts)
        eng.g1_compress_dev(d_pts, 4096, d_b)
        eng.g1_decompress_dev(d_b, 4096, d_back, d_st)
        assert np.array_equal(eng.download(d_b, (4096, 32), np.uint8), got)
        assert np.array_equal(eng.download(d_back, (4096, 8)), pts) and not eng.download(d_st, 4096, np.int32).any()
    finally:
        eng.dev_free(d)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------------
def test_random_strings_are_classified_like_the_reference(eng):
    rng = random.Random(0x72656675)
    data = [rng.randbytes(32) for _ in range(512)]
    data += [WR.P.to_bytes(32, "little"), (1 | 1 << 254).to_bytes(32, "little"), (1 << 255).to_bytes(32, "little"),
             (WR.P - 1).to_bytes(32, "little"), ((WR.P - 1) | 1 << 255).to_bytes(32, "little")]
    ref = [WR.decompress(b) for b in data]
    pts, st = eng.g1_decompress(b"".join(data))
    counts = [sum(1 for s, _ in ref[:512] if s == c) for c in (WR.OK, WR.NOT_CANONICAL, WR.OFF_CURVE)]
    print("\nrandom strings: ok / not canonical / off the curve =", counts)
    assert all(counts)
    assert [int(s) for s in st] == [s for s, _ in ref]
    for i, (s, pt) in enumerate(ref):
        assert [int(w) for w in pts[i]] == WR.point_words(pt if s == WR.OK else None), i
    assert [s for s, _ in ref[512:515]] == [WR.NOT_CANONICAL, WR.NOT_CANONICAL, WR.OFF_CURVE]


# ---- 3. the proof codec ----------------------------------------------------------------------------------------------------------------
def test_proof_bytes_are_the_reference_packing_and_round_trip(eng, world):
    from paillier_halo2_amd import verifier as PV

    vk = world["vk"]
    assert PV.proof_size_bytes(vk) == WR.proof_size(vk.n_adv, vk.n_lk) == world["handle"].wire_bytes
    for p, data in zip(world["proofs"], world["bytes"]):
        assert len(data) == PV.proof_size_bytes(vk)
        assert data == WR.proof_bytes(p.commitments, p.evals)
        back = PV.proof_from_bytes(eng, vk, data, handle=world["handle"])
        assert "h" not in back.evals and "constants" in back.evals
        assert set(back.commitments) == set(p.commitments) and set(back.evals) == set(p.evals) - {"h"}
        for f, a in back.commitments.items():
            assert np.array_equal(a, p.commitments[f]), f
        for f, a in back.evals.items():
            assert np.array_equal(a, p.evals[f]), f
    # without a handle of the caller's: the codec makes its own
    assert PV.proof_to_bytes(eng, vk, world["proofs"][0]) == world["bytes"][0]
    # the words of a decoded proof carry zero in the h(x) slot
    words, st = eng.proof_decode(world["handle"], np.frombuffer(world["bytes"][0], dtype=np.uint8))
    assert not st.any() and not words[0, -4:].any()
    assert np.array_equal(words[0, :-4], PV.pack_proof(vk, world["proofs"][0].commitments, world["proofs"][0].evals)[:-4])


# ---- 4. honest proofs ------------------------------------------------------------------------------------------------------------------
def test_honest_byte_proofs_verify(eng, world):
    from paillier_halo2_amd import verifier as PV

    vk, params, seeds, data = world["vk"], world["params"], world["seeds"], world["bytes"]
    assert PV.verify_batch_bytes(eng, params, vk, data, seeds) == (True, [True] * N_PROOFS)
    assert PV.verify_batch_bytes(eng, params, vk, data, seeds, handle=world["handle"]) == (True, [True] * N_PROOFS)
    decoded = [PV.proof_from_bytes(eng, vk, b, handle=world["handle"]) for b in data]
    assert PV.verify_batch(eng, params, vk, decoded, seeds) == (True, [True] * N_PROOFS)
    # the per-proof path (asked for A and B) agrees with the word entry point on the same proofs
    words = np.stack([PV.pack_proof(vk, p.commitments, p.evals) for p in world["proofs"]])
    ok_w, per_w, h_w, ab_w = eng.verify_batch_dev(world["handle"], words, seeds, want_h=True, want_ab=True)
    ok_b, per_b, h_b, ab_b = eng.verify_batch_bytes_dev(world["handle"], np.frombuffer(b"".join(data), dtype=np.uint8), seeds, want_h=True,
                                                        want_ab=True)
    assert (ok_b, per_b) == (ok_w, per_w) == (True, [True] * N_PROOFS)
    assert np.array_equal(h_b, h_w) and np.array_equal(ab_b, ab_w)
    assert PV.verify_batch_bytes(eng, params, vk, data[3:4], seeds[3:4]) == (True, [True])


# ---- 5. the tamper cases of test_gpu_verify_native.py, applied before encoding -------------------------------------------------------------
def test_tampered_proofs_get_the_same_verdict_through_bytes_as_through_words(eng, cref, world):
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
        data = PV.proof_to_bytes(eng, key, pr)
        assert data == WR.proof_bytes(pr.commitments, pr.evals), name
        through_bytes = PV.verify_batch_bytes(eng, world["params"], key, [data], [sd])
        through_words = PV.verify_batch_native(eng, world["params"], key, [pr], [sd])
        python_path = PV.verify_batch(eng, world["params"], key, [PV.proof_from_bytes(eng, key, data)], [sd])
        assert through_bytes == through_words == python_path == (False, [False]), name


# ---- 6. byte-level negatives -------------------------------------------------------------------------------------------------------------
def test_byte_level_negatives_flag_exactly_that_proof(eng, world):
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import verifier as PV

    vk, params, seeds, handle = world["vk"], world["params"], world["seeds"], world["handle"]
    n_own, n_ev = WR.proof_counts(vk.n_adv, vk.n_lk)
    ev0 = 32 * (n_own - 2)                                # the first evaluation's offset
    rng = random.Random(0x6e6567)

    def batch(which, edit):
        data = [bytearray(b) for b in world["bytes"]]
        edit(data[which])
        return [bytes(b) for b in data]

    def flip_eval(b):
        b[ev0 + 32 * 7] ^= 1                              # the low byte of an evaluation: the value moves by one, still below r
        assert WR.scalar_from_bytes(bytes(b[ev0 + 32 * 7:ev0 + 32 * 8]))[0] == WR.OK

    def eval_r(b):
        b[ev0 + 32 * 3:ev0 + 32 * 4] = WR.R.to_bytes(32, "little")

    def off_curve(b):
        b[32 * 2:32 * 3] = _off_curve_x(rng).to_bytes(32, "little")

    def sign(b):
        b[31] ^= 0x80                                     # -C for C: a valid point and a wrong proof
        assert WR.decompress(bytes(b[:32]))[0] == WR.OK

    # (proof index, edit, status pz_proof_decode gives that proof)
    for which, edit, status in ((2, flip_eval, 0), (4, eval_r, 1), (6, off_curve, 2), (0, sign, 0)):
        data = batch(which, edit)
        want = [i != which for i in range(N_PROOFS)]
        assert PV.verify_batch_bytes(eng, params, vk, data, seeds, handle=handle) == (False, want), edit.__name__
        _, st = eng.proof_decode(handle, np.frombuffer(b"".join(data), dtype=np.uint8))
        assert [int(s) for s in st] == [status if i == which else 0 for i in range(N_PROOFS)], edit.__name__
        if status:
            with pytest.raises(ValueError):
                PV.proof_from_bytes(eng, vk, data[which], handle=handle)
            # a refused proof is absent from the batch: no h(x), no A and B for it; the others' as without it
            _, per, h, ab = eng.verify_batch_bytes_dev(handle, np.frombuffer(b"".join(data), dtype=np.uint8), seeds, want_h=True, want_ab=True)
            assert per == want and not h[which].any() and not ab[which].any()
            rest = [i for i in range(N_PROOFS) if i != which]
            _, per_r, h_r, ab_r = eng.verify_batch_bytes_dev(handle, np.frombuffer(b"".join(data[i] for i in rest), dtype=np.uint8),
                                                             [seeds[i] for i in rest], want_h=True, want_ab=True)
            assert per_r == [True] * 7 and np.array_equal(h[rest], h_r) and np.array_equal(ab[rest], ab_r)
        else:
            decoded = [PV.proof_from_bytes(eng, vk, b, handle=handle) for b in data]
            assert PV.verify_batch(eng, params, vk, decoded, seeds) == (False, want), edit.__name__
    # a truncated proof is a malformed argument, not a verdict
    with pytest.raises((ValueError, pz.PzError)):
        PV.verify_batch_bytes(eng, params, vk, [world["bytes"][0][:-32]], seeds[:1], handle=handle)
    with pytest.raises((ValueError, pz.PzError)):
        PV.proof_from_bytes(eng, vk, world["bytes"][0][:-32], handle=handle)


# ---- 7. the compiled path ----------------------------------------------------------------------------------------------------------------
def test_compiled_prover_writes_wire_files_and_verify_wire_checks_them(eng, world, tmp_path):
    from paillier_halo2_amd import prover_job
    from paillier_halo2_amd import verifier as PV

    st, (nn, g, m, r, ng, nr) = world["st"], world["inputs"]
    rng = random.Random(0x6a6f64)
    job, proof = str(tmp_path / "job.bin"), str(tmp_path / "proof.bin")
    prover_job.write_job(job, st, world["starts"], BITS, 0, ng, nr, nn, g, [(m, r), (m, rng.randrange(1, nn))], world["s_tox"], seed=7,
                         proofs=2, tile=64)
    plain = str(tmp_path / "plain.bin")
    line0 = prover_job.run(job, plain)
    assert not os.path.exists(plain + ".vk") and not os.path.exists(plain + ".p0.bin")      # nothing more without the option
    line = prover_job.run(job, proof, env=dict(os.environ, PZ_PROVE_WIRE="1"))
    assert line["quotient_degree_ok"] is True and line["proofs"] == 2 and set(line) == set(line0)
    assert open(proof, "rb").read() == open(plain, "rb").read()                             # the record file is the same
    files = [proof + ".p0.bin", proof + ".p1.bin"]
    rec = prover_job.read_proofs(proof)
    vk = world["vk"]
    rvk = PV.VerifyingKey(K, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.n_sets, rec["vk/fixed"], rec["vk/sigma"])
    vk_file = open(proof + ".vk", "rb").read()
    assert vk_file == WR.vk_bytes(K, vk.blinding_factors, vk.n_adv, vk.n_lk, rec["vk/fixed"], rec["vk/sigma"]) == PV.vk_to_bytes(eng, rvk)
    for i, f in enumerate(files):
        com, ev = PV.proof_from_record(rec, "p%d/" % i, rvk)
        assert open(f, "rb").read() == WR.proof_bytes(com, ev), i

    csrc = os.path.join(ROOT, "paillier_halo2_amd", "csrc")
    exe = str(tmp_path / "verify_wire")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe,
                    os.path.join(ROOT, "paillier_halo2_amd", "host", "verify_wire.cpp"), "-L" + csrc, "-lpz_hip", "-Wl,-rpath," + csrc,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    run = lambda *a: subprocess.run([exe, *a], capture_output=True, text=True, timeout=300)
    r_ = run(proof + ".vk", world["params_path"], *files)
    assert r_.returncode == 0, r_.stderr
    out = json.loads(r_.stdout.strip().splitlines()[-1])
    print("\nverify_wire:", out)
    assert out["proofs"] == 2 and out["verified"] is True and out["per_proof"] == [True, True]
    n_own, _ = WR.proof_counts(vk.n_adv, vk.n_lk)
    b = bytearray(open(files[1], "rb").read())
    b[32 * (n_own - 2) + 32 * 5] ^= 1                    # one byte of one evaluation of proof 1 (still below r)
    bad = str(tmp_path / "bad.p1.bin")
    open(bad, "wb").write(bytes(b))
    r_ = run(proof + ".vk", world["params_path"], files[0], bad)
    assert r_.returncode == 1, r_.stderr
    out = json.loads(r_.stdout.strip().splitlines()[-1])
    assert out["verified"] is False and out["per_proof"] == [True, False]
    v = bytearray(vk_file)
    v[24 + 32:24 + 64] = _off_curve_x(random.Random(5)).to_bytes(32, "little")
    bad_vk = str(tmp_path / "bad.vk")
    open(bad_vk, "wb").write(bytes(v))
    assert run(bad_vk, world["params_path"], *files).returncode == 2
    assert run(proof + ".vk", world["params_path"], job).returncode == 2                    # not the size of a proof


# ---- 8. the key file ---------------------------------------------------------------------------------------------------------------------
def test_vk_round_trip(eng, world):
    from paillier_halo2_amd import verifier as PV

    vk = world["vk"]
    data = PV.vk_to_bytes(eng, vk)
    assert data == WR.vk_bytes(vk.k, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.fixed, vk.sigma)
    back = PV.vk_from_bytes(eng, data)
    assert (back.k, back.blinding_factors, back.n_adv, back.n_lk, back.n_sets) == (vk.k, vk.blinding_factors, vk.n_adv, vk.n_lk, vk.n_sets)
    assert np.array_equal(back.fixed, np.asarray(vk.fixed).reshape(-1, 8)) and np.array_equal(back.sigma, np.asarray(vk.sigma).reshape(-1, 8))
    assert PV.verify_batch_bytes(eng, world["params"], back, world["bytes"][:2], world["seeds"][:2]) == (True, [True, True])
    bad = bytearray(data)
    bad[24:56] = _off_curve_x(random.Random(9)).to_bytes(32, "little")
    with pytest.raises(ValueError):
        PV.vk_from_bytes(eng, bytes(bad))
    with pytest.raises(ValueError):
        PV.vk_from_bytes(eng, data[:-1])
