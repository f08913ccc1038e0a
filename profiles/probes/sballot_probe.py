"""Times the short-randomness ballot's K3 call.  Appends JSON lines to profiles/sballot_probe.jsonl (and
prints them).

    python sballot_probe.py [bits] [s_bits]     under a `bits`-bit key (default 2048) with s_bits = 448 by default, for b = 1 and
    b = 8 and K = 1, 4, 64, 256, 1024, on the same messages, one line per (b, K):
        sballot_dev_ms   pz_paillier_sballot_dev: K teams, each its g-chain of b bits, its hs-chain of s_bits bits and the product;
                         the records are left on the device
        ballot_dev_ms    pz_paillier_ballot_dev, what the library offered before for the same plaintexts: the g-chain, the r^n chain
                         over n's bits and the product; the records are left on the device
        steps_sballot / steps_ballot   the dependent mul_mod steps of one entry in either call: 2 b + 2 s_bits + 1 and 2 b + nr + 1

Every figure is the best of three, warmed, and ends in a synchronise.  Evidence, not a unit test.

Under its own time limit:
    timeout -k 10 600 python profiles/probes/sballot_probe.py 2048 448"""
import json
import math
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
    with open(os.path.join(ROOT, "profiles", "sballot_probe.jsonl"), "a") as f:
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
    n, g = P.synth_paillier_inputs(bits, 0x5e10)[:2]
    n2 = n * n
    Ln = -(-bits // 64)
    L = 2 * Ln
    sw = -(-s_bits // 64)
    lim = cref.int_to_limbs
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    nr = eng.ballot_steps_r(n)
    rng = random.Random(0x5e11)
    while True:
        x = rng.randrange(2, n)
        if math.gcd(x, n) == 1:
            break
    hs = pow((-x * x) % n, n, n2)
    n_w, g_w, hs_w = lim(n, Ln), lim(g, Ln), lim(hs, L)
    for b in (1, 8):
        per_s, per_b = 2 * b + 2 * s_bits + 1, 2 * b + nr + 1
        for K in (1, 4, 64, 256, 1024):
            ms = np.array([rng.randrange(1 << b) for _ in range(K)], dtype=np.uint64)
            ss = [rng.randrange(1 << s_bits) for _ in range(K)]
            rs = [rng.randrange(1, n) for _ in range(K)]
            s_w, r_w = np.stack([lim(s, sw) for s in ss]), np.stack([lim(r, Ln) for r in rs])
            d_s = torch.zeros((K, per_s, 4, L), dtype=torch.int64, device="cuda")
            d_b = torch.zeros((K, per_b, 4, L), dtype=torch.int64, device="cuda")
            short = lambda: eng.paillier_sballot_dev(Ln, n_w, g_w, hs_w, ms, s_w, b, s_bits, d_s.data_ptr(), K * per_s)
            full = lambda: eng.paillier_ballot_dev(Ln, n_w, g_w, ms, r_w, b, d_b.data_ptr(), K * per_b)
            short()
            c_s, t_s = _timed(eng, short)
            assert [cref.limbs_to_int(row) for row in c_s[:2]] == [pow(g, int(m), n2) * pow(hs, s, n2) % n2 for m, s in list(zip(ms, ss))[:2]]
            full()
            (c_b, _), t_b = _timed(eng, full)
            assert cref.limbs_to_int(c_b[0]) == pow(g, int(ms[0]), n2) * pow(rs[0], n, n2) % n2
            _emit({"probe": "k3", "bits": bits, "s_bits": s_bits, "b": b, "K": K, "steps_sballot": per_s, "steps_ballot": per_b,
                   "sballot_dev_ms": t_s, "ballot_dev_ms": t_b, "ratio": t_b / t_s, "steps_ratio": per_b / per_s})
            del d_s, d_b
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 2048, int(sys.argv[2]) if len(sys.argv) > 2 else 448))
