"""halo2 wire bytes on the device (csrc/pz_wire.hip).
  python profiles/probes/wire_probe.py [max B]      pz_verify_batch_bytes against pz_verify_batch at BASELINE config c2 (2048-bit n, k = 17),
        the same setup as verify_probe.py: wall time of the call for B = 1, 8, 32 honest proofs, the two entry points alternating in one
        process, warmed, as a range over repeats.  The word path gets the proofs already packed; the byte path gets the wire bytes.
  python profiles/probes/wire_probe.py --kernel     k_g1_decompress alone at n = 4936 (one c2 proof: 78 waves) and n = 2^20; run it under
        `rocprofv3 --kernel-trace --stats -- python profiles/probes/wire_probe.py --kernel` for the kernel's own time.  Prints the wall time
        per launch as well (stream-synchronised), and from n = 2^20 the field products per second: per accepted point the chain's 252
        squarings and 109 multiplications (the first pair works on one) and 7 products around it."""
import json, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import paillier_halo2_amd as pz

PRODUCTS_PER_POINT = 252 + 109 + 7      # f29_sqrt_candidate's loop + R517, to_261, x^2, x^3, y^2, y -> integer, y -> 256-domain
REPEATS = 5


def kernel_probe():
    eng = pz.Engine(0)
    rng = np.random.default_rng(0x77697265)
    out = {"kernel": "k_g1_decompress", "runs": []}
    for n in (4936, 1 << 20):
        sc = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        sc[:, 3] >>= 4                                        # any value below r is some scalar's Montgomery form
        d = eng.dev_alloc(n * (32 + 64 + 32 + 4))
        d_sc, d_pts, d_b, d_st = d, d + n * 32, d + n * 96, d + n * 128
        eng.upload(d_sc, sc)
        eng.g1_fixed_base_mul_dev(d_sc, n, d_pts)
        eng.g1_compress_dev(d_pts, n, d_b)
        eng.g1_decompress_dev(d_b, n, d_pts, d_st)            # warm-up
        eng.sync()
        assert not eng.download(d_st, n, np.int32).any()
        ms = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            eng.g1_decompress_dev(d_b, n, d_pts, d_st)
            eng.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        run = {"n": n, "wall_ms_min": round(min(ms), 3), "wall_ms_max": round(max(ms), 3),
               "products_per_s_from_wall_min": round(n * PRODUCTS_PER_POINT / (min(ms) * 1e-3), 0)}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        eng.dev_free(d)
    eng.close()
    print(json.dumps(out))


def batch_probe(max_b):
    import torch
    import bench_connected
    from paillier_halo2_amd import consts, prover, srs
    from paillier_halo2_amd import verifier as PV

    BITS, K, SEED = 2048, 17, 0x5043
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
    words = np.stack([PV.pack_proof(vk, p.commitments, p.evals) for p in proofs])
    t0 = time.perf_counter()
    data = eng.proof_encode(handle, words)
    encode_ms = (time.perf_counter() - t0) * 1e3
    out = {"config": "c2", "k": K, "n_adv": vk.n_adv, "n_lk": vk.n_lk, "proof_bytes": int(handle.wire_bytes), "proof_word_bytes": 8 * handle.proof_words,
           "encode_ms_for_max_b": round(encode_ms, 1), "runs": []}
    eng.verify_batch_dev(handle, words[:1], seeds[:1])            # warm-up: the library's workspaces
    eng.verify_batch_bytes_dev(handle, data[:1], seeds[:1])
    for B in (1, 8, 32):
        if B > max_b:
            continue
        tw, tb, same = [], [], True
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            rw = eng.verify_batch_dev(handle, words[:B], seeds[:B])
            t1 = time.perf_counter()
            rb = eng.verify_batch_bytes_dev(handle, data[:B], seeds[:B])
            t2 = time.perf_counter()
            tw.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
            same = same and rw[:2] == rb[:2] and rw[0] is True
        run = {"B": B, "words_ms": [round(min(tw), 1), round(max(tw), 1)], "bytes_ms": [round(min(tb), 1), round(max(tb), 1)],
               "same_verdicts_all_ok": same}
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
    handle.free()
    bl.free()
    bm.free()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernel":
        kernel_probe()
    else:
        batch_probe(int(sys.argv[1]) if len(sys.argv) > 1 else 32)
