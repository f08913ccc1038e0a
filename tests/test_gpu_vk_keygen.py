"""GPU: keygen_vk -- the verifying key derived from the circuit structure alone (include/pz.h: pz_g1_commit_mask_dev,
pz_permutation_sigma_part_dev, pz_vk_keygen[_dev]; verifier.VerifyingKey.from_structure; host/keygen_vk.cpp) at the reference's bench shape
(128-bit n, 64-bit limbs, k = 14, lookup_bits 13; the world of tests/test_gpu_verify_native.py): the mask commitment against the general MSM
and against a closed form, sigma by column ranges against the whole call, the derived key against the proving key's word for word and
against [sum_i col[i] L_i(s)] G in Python integers, the world's proofs under the derived key, tampered structures, and the compiled driver."""
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
N_PROOFS = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = pow(7, 1 << 28, R)          # halo2curves Fr::DELTA: 7 generates Fr's multiplicative group, r - 1 = 2^28 t


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(eng, cref, tmp_path_factory):
    """test_gpu_verify_native.py's recipe: structure on the CPU, SRS from a known scalar, a proving key and its proofs"""
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
        seed = b"vkgen-%d" % i
        proofs.append(prover.create_proof(pk, witness(), prover.HashTranscript(seed), seed=300 + i, tile=64))
        seeds.append(seed)
    del pk
    yield dict(st=st, starts=starts, vk=vk, params=vparams, params_path=path, proofs=proofs, seeds=seeds, s_tox=s_tox, bl=bl,
               inputs=(nn, g, m, r, ng, nr))
    bl.free()
    bm.free()


# ---- 1. the mask commitment ----------------------------------------------------------------------------------------------------------------
def _base_set(eng, cref, scalars):
    pts = eng.g1_fixed_base_mul(cref.fr_ints_to_mont(scalars))       # [a_i] G
    return eng.load_bases(pts)


def _check_masks(eng, cref, bases, a, mask, n, label):
    """mask: uint8 [n_cols][stride >= n].  The device result against (1) msm_dev of the fr_from_mask_dev columns and (2) [sum a_i mask_i] G in
    Python integers (oracle/pyref: no code shared with the library)."""
    import torch

    n_cols, stride = mask.shape
    d_mask = torch.from_numpy(mask).cuda()
    out = torch.full((n_cols, 12), -1, dtype=torch.int64, device="cuda")
    eng.g1_commit_mask_dev(bases, d_mask.data_ptr(), n_cols, n, stride, out.data_ptr())
    eng.sync()
    got = eng.g1_normalize(out.cpu().numpy().view(np.uint64))
    cols = torch.zeros((n_cols, max(n, 1), 4), dtype=torch.int64, device="cuda")
    for c in range(n_cols):
        eng.fr_from_mask_dev(d_mask[c].data_ptr(), n, cols[c].data_ptr())
    out2 = torch.zeros((n_cols, 12), dtype=torch.int64, device="cuda")
    eng.msm_dev(bases, cols.data_ptr(), n_cols, n, 4 * max(n, 1), out2.data_ptr())
    eng.sync()
    via_msm = eng.g1_normalize(out2.cpu().numpy().view(np.uint64))
    assert np.array_equal(got, via_msm), label + ": differs from msm_g1_dev of the fr_from_mask_dev columns"
    want = [P.g1_mul(P.G1_GEN, sum(a[i] for i in np.flatnonzero(mask[c, :n])) % R) for c in range(n_cols)]
    assert np.array_equal(got, cref.affine_ints_to_mont(want)), label + ": differs from [sum a_i mask_i] G"


def test_mask_commitment(eng, cref):
    rng = random.Random(0x6d61736b)
    nprng = np.random.default_rng(0x6d61736b)
    NP = 1024
    plain = [rng.randrange(1, R) for _ in range(NP)]
    special = list(plain)
    special[9] = special[5]                  # a repeated point (P + P inside one accumulator chain or across lanes)
    special[7] = R - special[3]              # a point and its negative
    special[11] = 0                          # an identity entry
    special[12] = special[5]                 # ... and the repeated point a third time
    for name, a in (("plain", plain), ("special", special)):
        bases = _base_set(eng, cref, a)
        try:
            def masks(n_cols, stride, density, values=False):
                m = (nprng.random((n_cols, stride)) < density).astype(np.uint8)
                if values:
                    m = m * nprng.integers(2, 256, size=m.shape, dtype=np.uint8)
                if name == "special":
                    m[:, [3, 5, 7, 9, 11, 12]] = 1 if not values else 0x80      # the special rows are all selected
                return np.ascontiguousarray(m)

            for n_cols in (1, 3, 70):
                lab = "%s n_cols %d " % (name, n_cols)
                z = np.zeros((n_cols, NP), dtype=np.uint8)
                if name == "plain":
                    _check_masks(eng, cref, bases, a, z, NP, lab + "density 0")
                one = z.copy()
                for c in range(n_cols):
                    one[c, (37 * c + 5) % NP] = 1
                _check_masks(eng, cref, bases, a, one, NP, lab + "one set row")
                _check_masks(eng, cref, bases, a, masks(n_cols, NP, 0.26), NP, lab + "density 0.26")
                _check_masks(eng, cref, bases, a, np.ones((n_cols, NP), dtype=np.uint8), NP, lab + "all ones")
                _check_masks(eng, cref, bases, a, masks(n_cols, NP, 0.26, values=True), NP, lab + "byte values other than 1")
                _check_masks(eng, cref, bases, a, masks(n_cols, NP, 0.26), 1000, lab + "n = 1000 of 1024 points")
                _check_masks(eng, cref, bases, a, masks(n_cols, 1031, 0.26), 1000, lab + "mask_stride 1031 > n = 1000")
                _check_masks(eng, cref, bases, a, masks(n_cols, 1040, 0.5), NP, lab + "mask_stride 1040 > n = 1024")
        finally:
            bases.free()
    # more rows than one workgroup's chunk: several partials per column and a ragged last chunk
    NB = 40000
    big = [rng.randrange(1, R) for _ in range(NB)]
    bases = _base_set(eng, cref, big)
    try:
        m = (nprng.random((3, NB)) < 0.26).astype(np.uint8)
        m[1, 16384:32768] = 0                                             # an empty chunk between two others
        _check_masks(eng, cref, bases, big, m, NB, "40000 rows")
        _check_masks(eng, cref, bases, big, m, 33000, "33000 of 40000 rows")
    finally:
        bases.free()


# ---- 2. sigma by parts ---------------------------------------------------------------------------------------------------------------------
def test_sigma_by_parts(eng, world):
    import torch

    import paillier_halo2_amd as pz
    from paillier_halo2_amd import consts
    from paillier_halo2_amd._lib import PZ_ERR_ASYNC

    st = world["st"]
    n, m = 1 << K, st.m
    M = consts.fr_mont_limbs
    omega, delta = M(consts.fr_omega(K)), M(DELTA)
    d_mc = torch.from_numpy(np.ascontiguousarray(st.map_col).view(np.int32)).cuda()
    d_mr = torch.from_numpy(np.ascontiguousarray(st.map_row).view(np.int32)).cuda()
    whole = torch.zeros((m, n, 4), dtype=torch.int64, device="cuda")
    eng.permutation_sigma_dev(d_mc.data_ptr(), d_mr.data_ptr(), m, K, omega, delta, whole.data_ptr(), 4 * n)
    eng.sync()
    assert m >= 20
    for lo, hi in ((0, 5), (5, 18), (18, m)):
        part = torch.full((hi - lo, n + 3, 4), -1, dtype=torch.int64, device="cuda")      # a stride of its own
        eng.permutation_sigma_part_dev(d_mc.data_ptr(), d_mr.data_ptr(), m, lo, hi - lo, K, omega, delta, part.data_ptr(), 4 * (n + 3))
        eng.sync()
        assert torch.equal(part[:, :n], whole[lo:hi]), (lo, hi)
        assert bool((part[:, n:] == -1).all()), (lo, hi)
    # an image in column m_total: clamped on the device, reported at the next synchronisation
    bad = d_mc.clone()
    bad[7, 123] = m
    part = torch.zeros((4, n, 4), dtype=torch.int64, device="cuda")
    eng.permutation_sigma_part_dev(bad.data_ptr(), d_mr.data_ptr(), m, 6, 4, K, omega, delta, part.data_ptr(), 4 * n)
    with pytest.raises(pz.PzError) as ei:
        eng.sync()
    assert ei.value.status == PZ_ERR_ASYNC
    eng.sync()                                                                            # the flag is cleared once reported
    # a range that does not lie inside the permutation is refused
    with pytest.raises(pz.PzError):
        eng.permutation_sigma_part_dev(d_mc.data_ptr(), d_mr.data_ptr(), m, m - 1, 2, K, omega, delta, part.data_ptr(), 4 * n)


# ---- 3. the key ----------------------------------------------------------------------------------------------------------------------------
def _device_structure(st):
    import dataclasses

    import torch

    return dataclasses.replace(st, selectors=torch.from_numpy(np.ascontiguousarray(st.selectors)).cuda(),
                               map_col=torch.from_numpy(np.ascontiguousarray(st.map_col).view(np.int32)).cuda(),
                               map_row=torch.from_numpy(np.ascontiguousarray(st.map_row).view(np.int32)).cuda())


def _same_key(a, b):
    return (a.k, a.blinding_factors, a.n_adv, a.n_lk, a.n_sets) == (b.k, b.blinding_factors, b.n_adv, b.n_lk, b.n_sets) and \
        np.array_equal(np.asarray(a.fixed).reshape(-1, 8), np.asarray(b.fixed).reshape(-1, 8)) and \
        np.array_equal(np.asarray(a.sigma).reshape(-1, 8), np.asarray(b.sigma).reshape(-1, 8))


def test_key_equals_the_proving_keys(eng, world):
    from paillier_halo2_amd import prover_native
    from paillier_halo2_amd import verifier as PV

    st, vk, bl = world["st"], world["vk"], world["bl"]
    nn, g, m, r, ng, nr = world["inputs"]
    assert st.m > 5 and st.m % 5 and st.m < 64           # tile 5 leaves a ragged last tile, tile 64 exceeds m
    dst = _device_structure(st)
    ns = prover_native.NativeStructure(eng, "encrypt", BITS, W, LB, K, exp_g=m, exp_r=nn)
    try:
        assert (ns.n_adv, ns.n_lk) == (st.n_adv, st.n_lk)
        for tile in (2, 5, 64):
            assert _same_key(PV.VerifyingKey.from_structure(eng, dst, bl, tile=tile), vk), ("device arrays", tile)
            assert _same_key(PV.VerifyingKey.from_structure(eng, st, bl, tile=tile), vk), ("host arrays", tile)
            assert _same_key(PV.VerifyingKey.from_structure(eng, ns, bl, tile=tile), vk), ("pz_structure handle", tile)
    finally:
        ns.free()


def test_key_is_the_commitment_of_the_structure(eng, cref, world):
    """every one of the F + m commitments equals [sum_i col[i] L_i(s)] G with the world's toxic scalar s, in Python integers from the CPU
    structure arrays: no device result enters the expectation"""
    from paillier_halo2_amd import verifier as PV

    st, bl, s = world["st"], world["bl"], world["s_tox"]
    n, A, m = 1 << K, st.n_adv, st.m
    omega = P.fr_omega(K)
    w = [1] * n
    for i in range(1, n):
        w[i] = w[i - 1] * omega % R
    scale = (pow(s, n, R) - 1) * pow(n, -1, R) % R
    L = [scale * w[i] % R * pow(s - w[i], -1, R) % R for i in range(n)]          # L_i(s) = (s^n - 1) w^i / (n (s - w^i))
    assert sum(L) % R == 1
    dp = [pow(DELTA, c, R) for c in range(m)]
    sel = np.asarray(st.selectors)
    want_fixed = [sum(L[i] for i in np.flatnonzero(sel[j])) % R for j in range(A)]
    want_fixed.append(sum(int(c) % R * L[i] for i, c in enumerate(st.constants)) % R)
    want_fixed.append(sum(i * L[i] for i in range(1 << LB)) % R)
    mc, mr = np.asarray(st.map_col), np.asarray(st.map_row)
    want_sigma = [sum(dp[int(c)] * w[int(r)] % R * L[i] for i, (c, r) in enumerate(zip(mc[j], mr[j]))) % R for j in range(m)]
    pts = lambda xs: cref.affine_ints_to_mont([P.g1_mul(P.G1_GEN, x) for x in xs])
    vk = PV.VerifyingKey.from_structure(eng, st, bl)
    assert np.array_equal(np.asarray(vk.fixed).reshape(-1, 8), pts(want_fixed))
    assert np.array_equal(np.asarray(vk.sigma).reshape(-1, 8), pts(want_sigma))


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------------
def test_proofs_verify_under_the_derived_key_and_not_under_a_tampered_one(eng, world):
    import dataclasses

    from paillier_halo2_amd import verifier as PV

    st, bl, params, proofs, seeds = world["st"], world["bl"], world["params"], world["proofs"], world["seeds"]
    vk = PV.VerifyingKey.from_structure(eng, st, bl)
    data = [PV.proof_to_bytes(eng, vk, p) for p in proofs]
    assert PV.verify_batch_native(eng, params, vk, proofs, seeds) == (True, [True] * N_PROOFS)
    assert PV.verify_batch_bytes(eng, params, vk, data, seeds) == (True, [True] * N_PROOFS)
    # one flipped selector byte
    sel = np.array(st.selectors, copy=True)
    j, i = 1, int(np.flatnonzero(sel[1])[3])
    sel[j, i] ^= 1
    # two map images swapped
    mc, mr = np.array(st.map_col, copy=True), np.array(st.map_row, copy=True)
    a, b = (0, 10), (2, 11)
    assert (mc[a], mr[a]) != (mc[b], mr[b])
    mc[a], mc[b] = mc[b], mc[a]
    mr[a], mr[b] = mr[b], mr[a]
    for name, bad_st in (("selector byte", dataclasses.replace(st, selectors=sel)), ("map images", dataclasses.replace(st, map_col=mc, map_row=mr))):
        bad = PV.VerifyingKey.from_structure(eng, bad_st, bl)
        assert not _same_key(bad, vk), name
        assert PV.verify_batch_native(eng, params, bad, proofs, seeds) == (False, [False] * N_PROOFS), name
        assert PV.verify_batch_bytes(eng, params, bad, data, seeds) == (False, [False] * N_PROOFS), name


# ---- 5. the compiled driver ----------------------------------------------------------------------------------------------------------------
def _gxx(src, exe):
    csrc = os.path.join(ROOT, "paillier_halo2_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe, os.path.join(ROOT, "paillier_halo2_amd", "host", src),
                    "-L" + csrc, "-lpz_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_compiled_keygen_vk_writes_the_provers_key_file(eng, world, tmp_path):
    from paillier_halo2_amd import layout, prover_job

    st, (nn, g, m, r, ng, nr) = world["st"], world["inputs"]
    rng = random.Random(0x6a6f64)
    job, proof = str(tmp_path / "job.bin"), str(tmp_path / "proof.bin")
    prover_job.write_job(job, st, world["starts"], BITS, 0, ng, nr, nn, g, [(m, r), (m, rng.randrange(1, nn))], world["s_tox"], seed=7,
                         proofs=2, tile=64)
    line = prover_job.run(job, proof, env=dict(os.environ, PZ_PROVE_WIRE="1"))
    assert line["quotient_degree_ok"] is True and line["proofs"] == 2
    exe, out = str(tmp_path / "keygen_vk"), str(tmp_path / "derived.vk")
    _gxx("keygen_vk.cpp", exe)
    r_ = subprocess.run([exe, world["params_path"], "encrypt", str(BITS), str(W), str(LB), str(K), str(layout.MINIMUM_ROWS_BENCH),
                         str(st.blinding_factors), "%x" % m, "%x" % nn, out], capture_output=True, text=True, timeout=300)
    assert r_.returncode == 0, r_.stderr
    info = json.loads(r_.stdout.strip().splitlines()[-1])
    print("\nkeygen_vk:", info)
    assert (info["n_adv"], info["n_lk"]) == (st.n_adv, st.n_lk) and info["structure_ms"] > 0 and info["vk_ms"] > 0
    assert open(out, "rb").read() == open(proof + ".vk", "rb").read()
    vexe = str(tmp_path / "verify_wire")
    _gxx("verify_wire.cpp", vexe)
    v = subprocess.run([vexe, out, world["params_path"], proof + ".p0.bin", proof + ".p1.bin"], capture_output=True, text=True, timeout=300)
    assert v.returncode == 0, v.stderr
    verdict = json.loads(v.stdout.strip().splitlines()[-1])
    assert verdict["verified"] is True and verdict["per_proof"] == [True, True]
    # a params file for another k is refused
    assert subprocess.run([exe, world["params_path"], "encrypt", str(BITS), str(W), str(LB), str(K + 1), str(layout.MINIMUM_ROWS_BENCH),
                           str(st.blinding_factors), "%x" % m, "%x" % nn, out], capture_output=True).returncode == 2
