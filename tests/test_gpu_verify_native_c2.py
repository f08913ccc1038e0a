"""GPU: the device batch verifier at BASELINE config c2 (2048-bit n, k = 17, lookup_bits 16): four proofs of the bench's connected
workload, verified by verifier.verify_batch (Python) and verify_batch_native (pz_verify_batch) -- the same verdicts for the honest batch
and for a batch with one proof tampered; both wall times are printed."""
import random
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BITS, K, SEED, N_PROOFS = 2048, 17, 0x5043, 4


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    e.bind_torch_stream()
    yield e
    e.close()


def test_c2_native_verdicts_equal_python(eng):
    import torch

    import bench_connected
    from paillier_halo2_amd import consts, prover, srs
    from paillier_halo2_amd import verifier as PV

    n = 1 << K
    s_tox = random.Random(SEED ^ 0x535253).randrange(2, consts.FR_R)
    M = consts.fr_mont_limbs
    d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    eng.srs_setup_g1_dev(K, M(s_tox), M(consts.fr_omega(K)), d_g.data_ptr(), d_gl.data_ptr())
    eng.sync()
    g0 = d_g[0].cpu().numpy().view(np.uint64).copy()
    g2, s_g2 = srs.setup_g2(eng, M(s_tox))
    bl, bm = eng.load_bases_dev(d_gl.data_ptr(), n), eng.load_bases_dev(d_g.data_ptr(), n)
    del d_g, d_gl
    wl = bench_connected.ConnectedWorkload(eng, torch, BITS, K, SEED, srs=(bl, bm, s_tox))
    try:
        proofs = []
        for i in range(N_PROOFS):
            pr = wl.step(timed=False, last=(i == N_PROOFS - 1))
            proofs.append(prover.Proof(commitments={k: v.copy() for k, v in pr.commitments.items()},
                                       evals={k: v.copy() for k, v in pr.evals.items()}))
        torch.cuda.synchronize()
        seeds = [b"pz-bench-%d" % i for i in range(N_PROOFS)]
        vk = PV.VerifyingKey.from_proving_key(wl.pk)
        params = PV.VerifierParams.from_parts(g0, g2, s_g2)
        tampered = list(proofs)
        t = prover.Proof(commitments=dict(proofs[2].commitments), evals=dict(proofs[2].evals))
        t.commitments["w2"] = t.commitments["w1"].copy()
        tampered[2] = t
        for name, batch, want in (("honest", proofs, (True, [True] * N_PROOFS)),
                                  ("one tampered", tampered, (False, [i != 2 for i in range(N_PROOFS)]))):
            t0 = time.perf_counter()
            py = PV.verify_batch(eng, params, vk, batch, seeds)
            t1 = time.perf_counter()
            nat = PV.verify_batch_native(eng, params, vk, batch, seeds)
            t2 = time.perf_counter()
            print("\nc2 %s batch of %d: verify_batch %.0f ms, verify_batch_native %.0f ms" % (name, N_PROOFS, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
            assert py == nat == want, name
    finally:
        wl.release()
        bl.free()
        bm.free()
