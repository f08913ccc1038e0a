"""Times the short-randomness mix's K3 call.  Appends JSON lines to profiles/smix_probe.jsonl (and prints
them).

    python smix_probe.py [bits] [s_bits]     under a `bits`-bit key (default 2048) with s_bits = 448 by default, for K = 1, 4, 64, 256,
    1024, on the same ciphertexts and switch bits, one line per K:
        smix_dev_ms   pz_paillier_smix_dev: the network's layers, then K teams, each its hs-chain of s_bits bits and the product; the
                      routes and records are left on the device
        mix_dev_ms    pz_paillier_mix_dev, what the library offered before for the same ciphertexts and bits: the same layers, then the
                      r^n chain over n's bits and the product; the routes and records are left on the device
        steps_smix / steps_mix   the dependent mul_mod steps of one output in either call: 2 s_bits + 1 and nr + 1

Every figure is the best of three, warmed, and ends in a synchronise.  Evidence, not a unit test.

Under its own time limit:
    timeout -k 10 600 python profiles/probes/smix_probe.py 2048 448"""
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
    with open(os.path.join(ROOT, "profiles", "smix_probe.jsonl"), "a") as f:
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
    from paillier_halo2_amd import mix

    cref.build()
    n = P.synth_paillier_inputs(bits, 0x5e20)[0]
    n2 = n * n
    Ln = -(-bits // 64)
    L = 2 * Ln
    sw = -(-s_bits // 64)
    lim = cref.int_to_limbs
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    nr = eng.ballot_steps_r(n)
    rng = random.Random(0x5e21)
    while True:
        x = rng.randrange(2, n)
        if math.gcd(x, n) == 1:
            break
    hs = pow((-x * x) % n, n, n2)
    n_w, hs_w = lim(n, Ln), lim(hs, L)
    per_s, per_m = 2 * s_bits + 1, nr + 1
    for K in (1, 4, 64, 256, 1024):
        cts = [rng.randrange(1, n2) for _ in range(K)]
        ss = [rng.randrange(1 << s_bits) for _ in range(K)]
        rs = [rng.randrange(1, n) for _ in range(K)]
        perm = mix.random_permutation(K, rand=rng.randrange)
        bits_w = eng.mix_route(perm)
        layers = eng.mix_layers(K)
        c_w = np.stack([lim(c, L) for c in cts])
        s_w, r_w = np.stack([lim(s, sw) for s in ss]), np.stack([lim(r, Ln) for r in rs])
        d_routes = torch.zeros((max(layers, 1), K, L), dtype=torch.int64, device="cuda")
        d_s = torch.zeros((K, per_s, 4, L), dtype=torch.int64, device="cuda")
        d_m = torch.zeros((K, per_m, 4, L), dtype=torch.int64, device="cuda")
        short = lambda: eng.paillier_smix_dev(Ln, n_w, hs_w, c_w, bits_w, s_w, s_bits, d_routes.data_ptr(), d_s.data_ptr(), K * per_s)
        full = lambda: eng.paillier_mix_dev(Ln, n_w, c_w, bits_w, r_w, d_routes.data_ptr(), d_m.data_ptr(), K * per_m)
        short()
        c_s, t_s = _timed(eng, short)
        assert [cref.limbs_to_int(row) for row in c_s[:2]] == [cts[p] * pow(hs, s, n2) % n2 for p, s in list(zip(perm, ss))[:2]]
        full()
        c_m, t_m = _timed(eng, full)
        assert cref.limbs_to_int(c_m[0]) == cts[perm[0]] * pow(rs[0], n, n2) % n2
        _emit({"probe": "k3", "bits": bits, "s_bits": s_bits, "K": K, "layers": layers, "steps_smix": per_s, "steps_mix": per_m,
               "smix_dev_ms": t_s, "mix_dev_ms": t_m, "ratio": t_m / t_s, "steps_ratio": per_m / per_s})
        del d_routes, d_s, d_m
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 2048, int(sys.argv[2]) if len(sys.argv) > 2 else 448))
