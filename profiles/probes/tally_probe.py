"""Times ONE tally at 2048-bit n, 64-bit limbs, lookup_bits 16, k = 17: python tally_probe.py B
Prints one JSON line: the K3 product tree, K4, structure + keygen, the proof, the device verifier's verdict, and the same product made
the only way the library could make it before -- B - 1 pz_mul_mod calls -- in the same run.  Evidence, not a unit test.

Both sizes, each GPU step under its own time limit, chained:
    timeout -k 10 600 python profiles/probes/tally_probe.py 64 && timeout -k 10 900 python profiles/probes/tally_probe.py 1024"""
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

BITS, W, LB, K = 2048, 64, 16, 17


def main(B: int):
    import torch

    import paillier_halo2_amd as pz
    from oracle import cref, pyref as P
    from paillier_halo2_amd import prover, prover_native, srs
    from paillier_halo2_amd import verifier as PV

    cref.build()
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    Ln, L, n_rows = BITS // W, 2 * (BITS // W), 1 << K
    rng = random.Random(0x7a60 + B)
    nn = P.synth_paillier_inputs(BITS, 0x7a60)[0]
    cts = [rng.randrange(1, nn * nn) for _ in range(B)]
    want = 1
    for c in cts:
        want = want * c % (nn * nn)
    lim = cref.int_to_limbs
    n_w, cts_w, n2_w = lim(nn, Ln), np.stack([lim(c, L) for c in cts]), lim(nn * nn, L)
    out = {"B": B, "bits": BITS, "k": K, "lookup_bits": LB}

    def timed(fn, reps=3):
        best = None
        for _ in range(reps):
            eng.sync()
            t0 = time.perf_counter()
            r = fn()
            eng.sync()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return r, best

    d_steps = torch.zeros((B - 1, 4, L), dtype=torch.int64, device="cuda")
    eng.paillier_tally_dev(Ln, n_w, cts_w, d_steps.data_ptr(), B - 1)          # warm-up: workspaces, code objects
    c, out["k3_tree_ms"] = timed(lambda: eng.paillier_tally_dev(Ln, n_w, cts_w, d_steps.data_ptr(), B - 1))
    assert cref.limbs_to_int(c) == want

    def loop():       # the same tree, one pz_mul_mod call per product
        cur = [cts_w[i] for i in range(B)]
        while len(cur) > 1:
            nxt = [eng.mul_mod(L, cur[2 * j], cur[2 * j + 1], n2_w)[1] for j in range(len(cur) // 2)]
            if len(cur) & 1:
                nxt.append(cur[-1])
            cur = nxt
        return cur[0]

    r, out["mul_mod_loop_ms"] = timed(loop, reps=1)
    assert cref.limbs_to_int(r) == want
    out["chain_step_equivalent_ms"] = round((B - 1) * 7.8e-3, 3)              # (B - 1) x the chain kernel's 7.8 us step
    t0 = time.perf_counter()
    ns = prover_native.NativeStructure(eng, "tally", BITS, W, LB, K, count=B, expose=True)
    eng.sync()
    out["structure_ms"] = (time.perf_counter() - t0) * 1e3
    out.update(n_adv=ns.n_adv, n_lk=ns.n_lk, n_public=ns.n_public, n_cells=ns.n_cells)
    F = lambda v: cref.fr_ints_to_mont([v % P.FR_R])[0]
    s_tox = rng.randrange(2, P.FR_R)
    d_g = torch.zeros((n_rows, 8), dtype=torch.int64, device="cuda")
    d_gl = torch.zeros((n_rows, 8), dtype=torch.int64, device="cuda")
    eng.srs_setup_g1_dev(K, F(s_tox), F(P.fr_omega(K)), d_g.data_ptr(), d_gl.data_ptr())
    eng.sync()
    g2, s_g2 = srs.setup_g2(eng, F(s_tox))
    params = PV.VerifierParams.from_parts(d_g[0].cpu().numpy().view(np.uint64), g2, s_g2)
    bl, bm = eng.load_bases_dev(d_gl.data_ptr(), n_rows), eng.load_bases_dev(d_g.data_ptr(), n_rows)
    t0 = time.perf_counter()
    key = ns.key(bl, bm)
    eng.sync()
    out["keygen_ms"] = (time.perf_counter() - t0) * 1e3
    d_mod = torch.from_numpy(n2_w.astype(np.int64)).cuda()
    inputs = np.concatenate([n_w, cts_w.reshape(-1), lim(want, L)])
    cols = torch.zeros((ns.m, n_rows, 4), dtype=torch.int64, device="cuda")

    def k4():
        eng.circuit_expand_cols_dev(3, Ln, W, LB, inputs, d_steps.data_ptr(), B - 1, 0, d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(),
                                    ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, n_rows)

    k4()
    _, out["k4_ms"] = timed(k4)
    inst = ns.gather_public(cols.data_ptr())
    assert inst == PV.public_inputs("tally", nn, None, want, cts=cts, enc_bits=BITS, limb_bits=W)
    seed = b"tally-probe"
    t0 = time.perf_counter()
    pr = prover_native.create_proof(key, cols.data_ptr(), prover.HashTranscript(seed), seed=1, instances=inst)
    eng.sync()
    out["proof_ms"] = (time.perf_counter() - t0) * 1e3
    vk_c = key.vk_commitments()
    vk = PV.VerifyingKey.from_structure(eng, ns, bl)
    assert np.array_equal(vk.sigma, vk_c["sigma"])
    ok, verdicts = PV.verify_batch_native(eng, params, vk, [pr], [seed], instances=[inst])
    out["verdict"] = int(bool(ok and verdicts[0] and pr.h_degree_ok))
    for f in list(out):
        if f.endswith("_ms"):
            out[f] = round(out[f], 3)
    print(json.dumps(out))
    key.free()
    ns.free()
    bl.free()
    bm.free()
    eng.close()
    return 0 if out["verdict"] == 1 else 1


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 64))
