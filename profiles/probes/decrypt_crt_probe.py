"""Times pz_paillier_decrypt_crt_dev against pz_paillier_decrypt_dev on the SAME handle and the SAME
ciphertexts, in one run and one GPU process: python decrypt_crt_probe.py [out.jsonl] [budget seconds]
At 2048, 3072 and 4096 bits, B in {1, 64, 256, 1024}, with and without r, a general g (the ginv^m chain runs).  The two paths
alternate (lambda, CRT, lambda, CRT, ...), each is warmed first, every figure is the best of three and ends in a synchronise.  The
outputs of the two paths are compared array for array, and the first plaintexts against Python's.  One JSON line per shape goes to
profiles/decrypt_crt_probe.jsonl (or the file named) and to stdout.  A shape is not started once the budget (default 400 s) is spent;
the line "stopped" says so.  Evidence, not a unit test.

Under a time limit of its own:
    timeout -k 10 600 python profiles/probes/decrypt_crt_probe.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BITS = (2048, 3072, 4096)
BATCHES = (1, 64, 256, 1024)


def main(out_path: str, budget_s: float):
    import torch

    import paillier_halo2_amd as pz
    from oracle import cref
    from tests import decrypt_ref as DR

    cref.build()
    t_start = time.perf_counter()
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    lim = cref.int_to_limbs

    def timed(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    with open(out_path, "a") as f:
        for bits in BITS:
            k = DR.key(bits, standard_g=False)
            n, g = k[0], k[1]
            p, q = DR.primes(bits)
            Ln = -(-bits // 64)
            n2 = n * n
            # max(BATCHES) ciphertexts from a few honest ones by the homomorphism (Python's own powers would take longer than the probe)
            ms, rs, cs = DR.encryptions(k, 4, 0xc479)
            cts, want = list(cs), list(ms)
            while len(cts) < max(BATCHES):
                i, j = len(cts) % 4, (len(cts) // 4) % len(cts)
                cts.append(cts[i] * cts[j] % n2)
                want.append((want[i] + want[j]) % n)
            words = np.stack([lim(c, 2 * Ln) for c in cts])
            sk = eng.paillier_sk(Ln, n, g, k[2], k[3], p, q)
            for B in BATCHES:
                if time.perf_counter() - t_start > budget_s:
                    line = json.dumps({"stopped": "budget of %g s spent before bits=%d B=%d" % (budget_s, bits, B)})
                    print(line)
                    f.write(line + "\n")
                    sk.free()
                    eng.close()
                    return 0
                d_cts = torch.from_numpy(words[:B].view(np.int64)).cuda()
                bufs = {}
                for path in ("lambda", "crt"):
                    bufs[path] = (torch.zeros((B, Ln), dtype=torch.int64, device="cuda"), torch.zeros((B, Ln), dtype=torch.int64, device="cuda"),
                                  torch.zeros((B,), dtype=torch.uint8, device="cuda"))
                out = {"bits": bits, "B": B}
                for want_r in (True, False):
                    def run(path):
                        d_m, d_r, d_f = bufs[path]
                        eng.paillier_decrypt_dev(sk, B, d_cts.data_ptr(), d_m.data_ptr(), d_r.data_ptr() if want_r else 0, d_f.data_ptr(),
                                                 crt=(path == "crt"))

                    best = {}
                    for path in ("lambda", "crt"):                              # warm both
                        timed(lambda: run(path))
                    for _ in range(3):                                          # alternating
                        for path in ("lambda", "crt"):
                            dt = timed(lambda: run(path))
                            best[path] = min(best.get(path, dt), dt)
                    tag = "with_r" if want_r else "m_only"
                    out["lambda_%s_ms" % tag], out["crt_%s_ms" % tag] = best["lambda"], best["crt"]
                    out["ratio_%s" % tag] = best["lambda"] / best["crt"]
                    a, b = bufs["lambda"], bufs["crt"]
                    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not bool(a[2].any())
                    if want_r:
                        assert torch.equal(a[1], b[1])
                    got = b[0][:4].cpu().numpy().view(np.uint64)
                    assert [cref.limbs_to_int(v) for v in got] == want[:min(B, 4)]
                out = {name: round(v, 3) if isinstance(v, float) else v for name, v in out.items()}
                line = json.dumps(out)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
            sk.free()
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decrypt_crt_probe.jsonl"),
                  float(sys.argv[2]) if len(sys.argv) > 2 else 400.0))
