"""The device batch verifier (pz_verify_batch via verifier.verify_batch_native) against the Python verifier (verifier.verify_batch) at
BASELINE config c2 (2048-bit n, k = 17): wall time for B = 1, 8, 32 proofs, honest and with one proof tampered (W2 := W1).  The host
transcript replay is part of what one more proof adds to an honest batch: (t(32) - t(1)) / 31, with its upload, kernels and MSM share,
bounds the replay per proof from above.  DESIGN.md section 15.
Usage: python profiles/probes/verify_probe.py [max B]   (default 32)"""
import json, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import paillier_halo2_amd as pz
import bench_connected
from paillier_halo2_amd import consts, prover, srs
from paillier_halo2_amd import verifier as PV

BITS, K, SEED = 2048, 17, 0x5043
max_b = int(sys.argv[1]) if len(sys.argv) > 1 else 32
eng = pz.Engine(0)
eng.bind_torch_stream()
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
proofs = []
for i in range(max_b):
    pr = wl.step(timed=False, last=(i == max_b - 1))
    proofs.append(prover.Proof(commitments={k: v.copy() for k, v in pr.commitments.items()}, evals={k: v.copy() for k, v in pr.evals.items()}))
torch.cuda.synchronize()
seeds = [b"pz-bench-%d" % i for i in range(max_b)]
vk = PV.VerifyingKey.from_proving_key(wl.pk)
wl.release()
params = PV.VerifierParams.from_parts(g0, g2, s_g2)
handle = PV.native_key(eng, params, vk)
PV.verify_batch_native(eng, params, vk, proofs[:1], seeds[:1], handle=handle)     # warm-up: the library's workspaces
out = {"config": "c2", "k": K, "n_adv": vk.n_adv, "n_lk": vk.n_lk, "runs": []}
for B in (1, 8, 32):
    if B > max_b:
        continue
    bad = list(proofs[:B])
    t = prover.Proof(commitments=dict(bad[B // 2].commitments), evals=dict(bad[B // 2].evals))
    t.commitments["w2"] = t.commitments["w1"].copy()
    bad[B // 2] = t
    for kind, batch in (("honest", proofs[:B]), ("one_tampered", bad)):
        t0 = time.perf_counter()
        nat = PV.verify_batch_native(eng, params, vk, batch, seeds[:B], handle=handle)
        t1 = time.perf_counter()
        py = PV.verify_batch(eng, params, vk, batch, seeds[:B])
        t2 = time.perf_counter()
        run = {"B": B, "batch": kind, "native_ms": round((t1 - t0) * 1e3, 1), "python_ms": round((t2 - t1) * 1e3, 1),
               "same_verdicts": nat == py, "all_ok": nat[0]}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
honest = {r["B"]: r["native_ms"] for r in out["runs"] if r["batch"] == "honest"}
if len(honest) > 1:
    hi, lo = max(honest), min(honest)
    out["marginal_ms_per_proof"] = round((honest[hi] - honest[lo]) / (hi - lo), 2)          # replay + upload + kernels + MSM share
    out["replay_share_at_max_b_at_most"] = round(hi * out["marginal_ms_per_proof"] / honest[hi], 3)
handle.free()
bl.free()
bm.free()
print(json.dumps(out))
