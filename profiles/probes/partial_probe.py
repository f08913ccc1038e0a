"""Times one trustee's partial decryptions and the combiner: python partial_probe.py K bits
Appends one JSON line to profiles/partial_probe.jsonl (and prints it): pz_paillier_partial_dev for K ciphertexts under a share of
2 * bits bits with the records left on the device (K + 1 chains of 4 * bits steps, one launch), in the same run the route the library
had before -- one pz_paillier_trace(c^2, theta) per chain, values only --, and pz_paillier_combine_dev for T = 3 and T = 16 trustees
over the same K.  Every figure is the best of three, warmed, and ends in a synchronise.  The trace route is a serial loop: beyond 4
chains it is timed on 4 and scaled, and the line says so.  Evidence, not a unit test.

Each GPU step under its own time limit, chained:
    timeout -k 10 300 python profiles/probes/partial_probe.py 1 2048 && timeout -k 10 300 python profiles/probes/partial_probe.py 4 2048 && ..
(K = 1, 4, 64, 255 is the table of section 15.11; the records of K = 255 at 2048 bits are 4.3 GB of device memory)"""
import json
import math
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(K: int, bits: int):
    import torch

    import paillier_halo2_amd as pz
    from oracle import cref
    from paillier_halo2_amd import keys
    from tests import decrypt_ref as DR

    cref.build()
    p, q = DR.primes(bits)
    rng = random.Random(0x7a90 + K)
    t0 = time.perf_counter()
    key, shares = keys.deal_shares(p, q, 16, rand=rng.randrange)
    deal_ms = (time.perf_counter() - t0) * 1e3
    n, n2 = key.n, key.n * key.n
    N = n * ((p - 1) * (q - 1) // math.gcd(p - 1, q - 1))
    Ln = -(-bits // 64)
    L = 2 * Ln
    e_bits = 2 * bits
    lim = cref.int_to_limbs
    # K ciphertexts from two honest ones by the homomorphism (Python's own powers would take longer than the probe)
    ms = [12345, n - 1]
    cts = [pow(key.g, m, n2) * pow(rng.randrange(1, n), n, n2) % n2 for m in ms]
    while len(cts) < K:
        i, j = len(cts) % 2, len(cts) // 2 % len(cts)
        cts.append(cts[i] * cts[j] % n2)
        ms.append((ms[i] + ms[j]) % n)
    cts, ms = cts[:K], ms[:K]
    cts_w = np.stack([lim(c, L) for c in cts])
    n_w, v_w = lim(n, Ln), lim(key.v, L)
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    out = {"K": K, "bits": bits, "e_bits": e_bits, "deal_16_shares_python_ms": deal_ms}

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

    n_rec = eng.partial_records(K, e_bits)
    d_steps = torch.empty((n_rec, 4, L), dtype=torch.int64, device="cuda")
    out["records_bytes"] = n_rec * 4 * L * 8
    th_w = lim(shares[0], L)
    partial = lambda: eng.paillier_partial_dev(Ln, n_w, v_w, th_w, cts_w, e_bits, d_steps.data_ptr(), n_rec)
    partial()                                                                   # warm-up: workspaces, code objects
    (h, u), out["partial_dev_ms"] = timed(partial)
    assert cref.limbs_to_int(h) == key.hs[0]
    assert cref.limbs_to_int(u[0]) == pow(cts[0] * cts[0] % n2, shares[0], n2)
    del d_steps
    # the parent's route: one trace call per chain (the base squared on the host), values only
    Ct = min(K + 1, 4)
    n2_w = lim(n2, L)
    bases = [key.v] + [c * c % n2 for c in cts]
    bases_w = [lim(b, L) for b in bases[:Ct]]

    def trace_route():
        return [cref.limbs_to_int(eng.paillier_trace(L, n2_w, b, th_w, L, want_steps=False)[0]) for b in bases_w]

    trace_route()
    got, dt = timed(trace_route)
    assert got == [cref.limbs_to_int(h)] + [cref.limbs_to_int(x) for x in u[: Ct - 1]]
    out["trace_route_ms"] = dt * (K + 1) / Ct
    out["trace_route_timed_on"] = Ct
    # the combiner: every trustee's partials of the K ciphertexts (Python's powers for T = 16 would take minutes: the partials of the
    # first two ciphertexts are exact, the rest follow from them by the homomorphism u(c c') = u(c) u(c'))
    for T in (3, 16):
        sub = shares[: T - 1]
        last = (sum(shares) - sum(sub)) % N             # T shares of the same theta
        parts = []
        for s in sub + [last]:
            us = [pow(c * c % n2, s, n2) for c in cts[:2]]
            while len(us) < K:
                i, j = len(us) % 2, len(us) // 2 % len(us)
                us.append(us[i] * us[j] % n2)
            parts.append(np.stack([lim(x, L) for x in us[:K]]))
        d_parts = torch.from_numpy(np.stack(parts).astype(np.int64)).cuda()
        d_m = torch.zeros((K, Ln), dtype=torch.int64, device="cuda")
        d_fl = torch.zeros(K, dtype=torch.uint8, device="cuda")
        comb = lambda: eng.paillier_combine_dev(Ln, n_w, lim(key.mu2, Ln), K, T, d_parts.data_ptr(), d_m.data_ptr(), d_fl.data_ptr())
        comb()
        _, out["combine_dev_T%d_ms" % T] = timed(comb)
        assert not d_fl.cpu().numpy().any()
        assert [cref.limbs_to_int(r) for r in d_m.cpu().numpy().view(np.uint64)] == ms
    eng.close()
    out = {f: round(v, 3) if isinstance(v, float) else v for f, v in out.items()}
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "partial_probe.jsonl"), "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 2048))
