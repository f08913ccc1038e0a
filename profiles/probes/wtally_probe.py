"""Times ONE weighted tally at 2048-bit n, 64-bit limbs, lookup_bits 16: python wtally_probe.py B W [k | k3]
Prints one JSON line: K3 (the whole call, the tree alone as a tally over the powers, the chains by difference), K4, structure, keygen,
the proof, the device verifier's verdict, and the same chains made the only way the library could make them before -- one
pz_paillier_trace call per ciphertext -- in the same run.  k defaults to the smallest whose column count stays below 64; `k3` in its
place stops after the K3 figures (the sweep over B that asks whether one team per chain is right when chains are few).  Evidence, not a
unit test.

Each GPU step under its own time limit, chained:
    timeout -k 10 600 python profiles/probes/wtally_probe.py 64 16 && timeout -k 10 600 python profiles/probes/wtally_probe.py 4 16"""
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

BITS, W, LB = 2048, 64, 16


def main(B: int, WB: int, K: int = 0):
    import torch

    import paillier_halo2_amd as pz
    from oracle import cref, pyref as P
    from paillier_halo2_amd import layout, prover, prover_native, srs
    from paillier_halo2_amd import verifier as PV

    cref.build()
    Ln, L = BITS // W, 2 * (BITS // W)
    cc = layout.circuit_cells("wtally", Ln, W, LB, count=B, w_bits=WB)
    k3_only = K < 0
    if K <= 0:
        K = LB + 1
        while layout.row_budget(K).columns_for(cc.advice) >= 64:
            K += 1
    n_rows = 1 << K
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    rng = random.Random(0x3a60 + 64 * B + WB)
    nn = P.synth_paillier_inputs(BITS, 0x3a60)[0]
    n2 = nn * nn
    cts = [rng.randrange(1, n2) for _ in range(B)]
    weights = [rng.randrange(1 << WB) for _ in range(B)]
    powers = [pow(c, w, n2) for c, w in zip(cts, weights)]
    want = 1
    for p in powers:
        want = want * p % n2
    lim = cref.int_to_limbs
    n_w, cts_w, n2_w = lim(nn, Ln), np.stack([lim(c, L) for c in cts]), lim(n2, L)
    w_w = np.array(weights, dtype=np.uint64)
    out = {"B": B, "w_bits": WB, "bits": BITS, "k": K, "lookup_bits": LB}

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

    ns_rec = 2 * B * WB + B - 1
    d_steps = torch.zeros((ns_rec, 4, L), dtype=torch.int64, device="cuda")
    run = lambda: eng.paillier_wtally_dev(Ln, n_w, cts_w, w_w, WB, d_steps.data_ptr(), ns_rec)
    run()                                                                       # warm-up: workspaces, code objects
    c, out["k3_total_ms"] = timed(run)
    assert cref.limbs_to_int(c) == want
    out["k3_tree_ms"] = 0.0
    if B > 1:       # the tree alone: the tally of the powers (its own n^2 setup included, as in the whole call)
        pw_w = np.stack([lim(p, L) for p in powers])
        d_tree = torch.zeros((B - 1, 4, L), dtype=torch.int64, device="cuda")
        eng.paillier_tally_dev(Ln, n_w, pw_w, d_tree.data_ptr(), B - 1)
        c2, out["k3_tree_ms"] = timed(lambda: eng.paillier_tally_dev(Ln, n_w, pw_w, d_tree.data_ptr(), B - 1))
        assert cref.limbs_to_int(c2) == want
    out["k3_chains_ms_by_difference"] = out["k3_total_ms"] - out["k3_tree_ms"]

    def loop():       # the same chains, one pz_paillier_trace call per ciphertext (the reference schedule: bits + set bits steps each)
        return [eng.paillier_trace(L, n2_w, cts_w[i], np.array([weights[i]], dtype=np.uint64), 1, want_steps=False)[0] for i in range(B)]

    rs, out["trace_loop_ms"] = timed(loop, reps=1)
    assert [cref.limbs_to_int(r) for r in rs] == powers
    out["trace_loop_steps"] = sum(w.bit_length() + bin(w).count("1") for w in weights)      # the reference schedule's step count
    out["wtally_steps"] = ns_rec
    if k3_only:
        del out["k"]
        print(json.dumps({f: round(v, 3) if isinstance(v, float) else v for f, v in out.items()}))
        eng.close()
        return 0
    t0 = time.perf_counter()
    ns = prover_native.NativeStructure(eng, "wtally", BITS, W, LB, K, count=B, w_bits=WB, expose=True)
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
    inputs = np.concatenate([n_w, cts_w.reshape(-1), w_w, lim(want, L)])
    cols = torch.zeros((ns.m, n_rows, 4), dtype=torch.int64, device="cuda")

    def k4():
        eng.circuit_expand_cols_dev(4, Ln, W, LB, inputs, d_steps.data_ptr(), 2 * B * WB, B - 1, d_mod.data_ptr(), cols.data_ptr(),
                                    cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, n_rows)

    k4()
    _, out["k4_ms"] = timed(k4)
    inst = ns.gather_public(cols.data_ptr())
    assert inst == PV.public_inputs("wtally", nn, None, want, cts=cts, weights=weights, enc_bits=BITS, limb_bits=W)
    seed = b"wtally-probe"
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
        if f.endswith("_ms") or f.endswith("_difference"):
            out[f] = round(out[f], 3)
    print(json.dumps(out))
    key.free()
    ns.free()
    bl.free()
    bm.free()
    eng.close()
    return 0 if out["verdict"] == 1 else 1


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 64, int(sys.argv[2]) if len(sys.argv) > 2 else 16,
                  (-1 if sys.argv[3] == "k3" else int(sys.argv[3])) if len(sys.argv) > 3 else 0))
