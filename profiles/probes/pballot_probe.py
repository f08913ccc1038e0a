"""Times the packed ballot's K3 call.  Appends JSON lines to profiles/pballot_probe.jsonl (and prints them).

    python pballot_probe.py [bits] [s_bits]     under a `bits`-bit key (default 2048) with s_bits = 448 by default and b = 1, for
    K = 2, 8, 32 slots and R = 1, 32, 128, 1024 ciphertexts wherever R K <= 1024 (the call's own bound; the greatest R a K admits, 1024 / K,
    is added), one line per (K, R):
        pballot_dev_ms   pz_paillier_pballot_dev: R teams, each its K slot chains of b bits, its hs-chain of s_bits bits and the K
                         folds; the records are left on the device
        sballot_dev_ms   pz_paillier_sballot_dev on the same R K votes as R K separate ciphertexts, what the library offered before:
                         R K teams, each a g-chain, an hs-chain and one product; the records are left on the device
        steps_pballot / steps_sballot   the dependent mul_mod steps of one team in either call: 2 b K + 2 s_bits + K and
                         2 b + 2 s_bits + 1
        expect_ratio     what DESIGN.md section 15.21 states BEFORE the run for sballot_dev_ms / pballot_dev_ms: the teams of either
                         call run in ceil(teams / 256) waves of one chain each over the 256 compute units

Every figure is the best of three, warmed, and ends in a synchronise.  Evidence, not a unit test.

Under its own time limit:
    timeout -k 10 600 python profiles/probes/pballot_probe.py 2048 448"""
import json
import math
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CUS = 256


def _emit(out):
    out = {f: round(v, 3) if isinstance(v, float) else v for f, v in out.items()}
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(ROOT, "profiles", "pballot_probe.jsonl"), "a") as f:
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


def main(bits: int, s_bits: int):
    import torch

    import paillier_halo2_amd as pz
    from oracle import cref
    from oracle import pyref as P

    cref.build()
    n, g = P.synth_paillier_inputs(bits, 0x9b10)[:2]
    n2 = n * n
    Ln = -(-bits // 64)
    L = 2 * Ln
    sw = -(-s_bits // 64)
    lim = cref.int_to_limbs
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    rng = random.Random(0x9b11)
    while True:
        x = rng.randrange(2, n)
        if math.gcd(x, n) == 1:
            break
    hs = pow((-x * x) % n, n, n2)
    n_w, g_w, hs_w = lim(n, Ln), lim(g, Ln), lim(hs, L)
    b, w = 1, 16
    per_s = 2 * b + 2 * s_bits + 1
    for K in (2, 8, 32):
        gs = [pow(g, 1 << (j * w), n2) for j in range(K)]
        gs_w = np.stack([lim(gj, L) for gj in gs])
        per_p = 2 * b * K + 2 * s_bits + K
        for Rn in sorted({r for r in (1, 32, 128, 1024, 1024 // K) if r * K <= 1024}):
            vs = np.array([[rng.randrange(1 << b) for _ in range(K)] for _ in range(Rn)], dtype=np.uint64)
            ss = [rng.randrange(1 << s_bits) for _ in range(Rn * K)]
            s_w = np.stack([lim(s, sw) for s in ss])
            d_p = torch.zeros((Rn, per_p, 4, L), dtype=torch.int64, device="cuda")
            d_s = torch.zeros((Rn * K, per_s, 4, L), dtype=torch.int64, device="cuda")
            packed = lambda: eng.paillier_pballot_dev(Ln, n_w, hs_w, gs_w, vs, s_w[:Rn], b, s_bits, d_p.data_ptr(), Rn * per_p)
            apart = lambda: eng.paillier_sballot_dev(Ln, n_w, g_w, hs_w, vs.reshape(-1), s_w, b, s_bits, d_s.data_ptr(), Rn * K * per_s)
            packed()
            c_p, t_p = _timed(eng, packed)
            M0 = sum(int(v) << (j * w) for j, v in enumerate(vs[0]))
            assert cref.limbs_to_int(c_p[0]) == pow(g, M0, n2) * pow(hs, ss[0], n2) % n2
            apart()
            c_s, t_s = _timed(eng, apart)
            assert cref.limbs_to_int(c_s[0]) == pow(g, int(vs[0, 0]), n2) * pow(hs, ss[0], n2) % n2
            expect = (math.ceil(Rn * K / CUS) * per_s) / (math.ceil(Rn / CUS) * per_p)
            _emit({"probe": "k3", "bits": bits, "s_bits": s_bits, "b": b, "K": K, "R": Rn, "votes": Rn * K, "steps_pballot": per_p,
                   "steps_sballot": per_s, "pballot_dev_ms": t_p, "sballot_dev_ms": t_s, "ratio": t_s / t_p, "expect_ratio": expect,
                   "expect_pballot_ms": math.ceil(Rn / CUS) * per_p * 7.6e-3, "expect_sballot_ms": math.ceil(Rn * K / CUS) * per_s * 7.6e-3})
            del d_p, d_s
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 2048, int(sys.argv[2]) if len(sys.argv) > 2 else 448))
