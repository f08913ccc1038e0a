"""Times the ballot.  Appends JSON lines to profiles/ballot_probe.jsonl (and prints them).

    python ballot_probe.py k3 [bits]         pz_paillier_ballot_dev at b = 1 and b = 8, K = 1, 2, 8, 64, 256, 1024, and in the same run
                                             the route the library had before: pz_paillier_encrypt_uniform_dev(batch = K, m_bits = b)
                                             on the same inputs (n and g copied per instance).  One line per (b, K).
    python ballot_probe.py proof [bits] [k]  ONE connected ballot proof (K = 2, b = 1) by the native stepper -- K3, K4 and create_proof,
                                             key generation aside -- and, from the same run, one connected uniform-shape encrypt (c2u)
                                             proof at the same k; device memory in use after each.  One line.

Every figure is the best of three, warmed, and ends in a synchronise.  Evidence, not a unit test.

Each GPU step under its own time limit, chained:
    timeout -k 10 300 python profiles/probes/ballot_probe.py k3 2048 && timeout -k 10 900 python profiles/probes/ballot_probe.py proof 2048 17"""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _emit(out):
    out = {f: round(v, 3) if isinstance(v, float) else v for f, v in out.items()}
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "ballot_probe.jsonl"), "a") as f:
        f.write(line + "\n")


def _timed(eng, fn, reps=3):
    best = None
    for _ in range(reps):
        eng.sync()
        t0 = time.perf_counter()
        r = fn()
        eng.sync()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return r, best


def k3(bits: int):
    import torch

    import paillier_halo2_amd as pz
    from oracle import cref
    from oracle import pyref as P

    cref.build()
    n, g = P.synth_paillier_inputs(bits, 0x6b60)[:2]
    Ln = -(-bits // 64)
    L = 2 * Ln
    lim = cref.int_to_limbs
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    nr = eng.ballot_steps_r(n)
    rng = random.Random(0x6b61)
    n_w, g_w = lim(n, Ln), lim(g, Ln)
    for b in (1, 8):
        per = 2 * b + nr + 1
        for K in (1, 2, 8, 64, 256, 1024):
            ms = [rng.randrange(1 << b) for _ in range(K)]
            rs = np.stack([lim(rng.randrange(1, n), Ln) for _ in range(K)])
            m_w = np.zeros((K, Ln), dtype=np.uint64)
            m_w[:, 0] = ms
            d_steps = torch.zeros((K, per, 4, L), dtype=torch.int64, device="cuda")
            rep_n, rep_g = np.stack([n_w] * K), np.stack([g_w] * K)
            ballot = lambda: eng.paillier_ballot_dev(Ln, n_w, g_w, ms, rs, b, d_steps.data_ptr(), K * per)
            uniform = lambda: eng.paillier_encrypt_uniform_dev(Ln, b, rep_n, rep_g, m_w, rs, d_steps.data_ptr(), per)
            ballot()
            (c, _), t_ballot = _timed(eng, ballot)
            rec_b = d_steps[:, -1].cpu().numpy()
            uniform()
            (cu, _, _), t_uniform = _timed(eng, uniform)
            assert np.array_equal(c, cu) and np.array_equal(rec_b, d_steps[:, -1].cpu().numpy())
            assert cref.limbs_to_int(c[0]) == P.paillier_enc_native(n, g, ms[0], cref.limbs_to_int(rs[0]))
            _emit({"probe": "k3", "bits": bits, "m_bits": b, "K": K, "n_steps_r": nr, "ballot_dev_ms": t_ballot, "encrypt_uniform_dev_ms": t_uniform})
            del d_steps
    eng.close()
    return 0


def proof(bits: int, k: int):
    import torch

    import paillier_halo2_amd as pz
    from oracle import cref
    from oracle import pyref as P
    from paillier_halo2_amd import prover, prover_native

    cref.build()
    W, lb, K, b = 64, k - 1, 2, 1
    n, g, m_u, r_u = P.synth_paillier_inputs(bits, 0x6b62)
    Ln = bits // W
    L = 2 * Ln
    lim = cref.int_to_limbs
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    rows = 1 << k
    F = lambda v: cref.fr_ints_to_mont([v % P.FR_R])[0]
    d_g = torch.zeros((rows, 8), dtype=torch.int64, device="cuda")
    d_gl = torch.zeros((rows, 8), dtype=torch.int64, device="cuda")
    eng.srs_setup_g1_dev(k, F(0x6b63), F(P.fr_omega(k)), d_g.data_ptr(), d_gl.data_ptr())
    eng.sync()
    bl, bm = eng.load_bases_dev(d_gl.data_ptr(), rows), eng.load_bases_dev(d_g.data_ptr(), rows)
    d_mod = torch.from_numpy(lim(n * n, L).astype(np.int64)).cuda()
    nr = eng.ballot_steps_r(n)
    out = {"probe": "proof", "bits": bits, "k": k, "K": K, "m_bits": b}
    mem = lambda: (torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]) / 2 ** 30

    def run(kind):
        if kind == "ballot":
            ns = prover_native.NativeStructure(eng, "ballot", bits, W, lb, k, exp_r=n, count=K, m_bits=b, expose=True)
            per = 2 * b + nr + 1
            ms, rs = [1, 0], [r_u, r_u ^ 5]
            rs_w = np.stack([lim(r, Ln) for r in rs])
            n_rec = K * per
        else:
            ns = prover_native.NativeStructure(eng, "encrypt_uniform", bits, W, lb, k, exp_r=n, expose=True)
            n_rec = 2 * bits + nr + 1
        key = ns.key(bl, bm)
        d_steps = torch.zeros((n_rec, 4, L), dtype=torch.int64, device="cuda")
        cols = torch.zeros((ns.m, rows, 4), dtype=torch.int64, device="cuda")

        def one():
            if kind == "ballot":
                c, _ = eng.paillier_ballot_dev(Ln, lim(n, Ln), lim(g, Ln), ms, rs_w, b, d_steps.data_ptr(), n_rec)
                inputs = np.concatenate([lim(n, Ln), lim(g, Ln), np.array(ms, dtype=np.uint64), rs_w.reshape(-1), c.reshape(-1)])
                eng.ballot_expand_cols_dev(Ln, W, lb, K, b, nr, inputs, d_steps.data_ptr(), d_mod.data_ptr(), cols.data_ptr(),
                                           cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, rows)
            else:
                c, _, _ = eng.paillier_encrypt_uniform_dev(Ln, bits, lim(n, Ln), lim(g, Ln), lim(m_u, Ln), lim(r_u, Ln), d_steps.data_ptr(), n_rec)
                inputs = np.concatenate([lim(n, Ln), lim(g, Ln), lim(m_u, Ln), lim(r_u, Ln), c.reshape(-1)])
                eng.circuit_expand_cols_dev(2, Ln, W, lb, inputs, d_steps.data_ptr(), 2 * bits, nr, d_mod.data_ptr(), cols.data_ptr(),
                                            cols[ns.n_adv].data_ptr(), ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, rows)
            inst = ns.gather_public(cols.data_ptr())
            return prover_native.create_proof(key, cols.data_ptr(), prover.HashTranscript(b"ballot-probe"), seed=3, instances=inst)

        assert one().h_degree_ok
        pr, dt = _timed(eng, one)
        assert pr.h_degree_ok
        out[kind + "_proof_ms"] = dt
        out[kind + "_advice_columns"] = ns.n_adv
        out[kind + "_device_gib"] = mem()
        key.free()
        ns.free()
        del d_steps, cols
        torch.cuda.empty_cache()

    run("ballot")
    run("encrypt_uniform")
    _emit(out)
    eng.close()
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "k3"
    bits = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    sys.exit(k3(bits) if mode == "k3" else proof(bits, int(sys.argv[3]) if len(sys.argv) > 3 else 17))
