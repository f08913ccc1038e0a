"""Times the mix.  Appends JSON lines to profiles/mix_probe.jsonl (and prints them).

    python mix_probe.py [bits]     pz_paillier_mix_dev at K = 1, 4, 64, 256, 1024 under a `bits`-bit key (default 2048), one line per K:
        mix_dev_ms       the whole call: the 2 log2(K) - 1 route launches, then the K r^n chains and products in one launch
        route_ms         the route apart: the same call at the same limb count and K under the modulus n = 3 on zero ciphertexts --
                         the same launches moving the same words, every chain cut to five short steps
        rerand_ms        mix_dev_ms - route_ms
        parent_ms        what the library offered for the same outputs before: pz_paillier_ballot_dev with m = 0, b = 1 for the
                         r_i^n (parent_chains_ms), then the K products c_perm(i) * r_i^n as K calls of pz_mul_mod, one k_mul_mod
                         launch each (parent_products_ms) -- the permutation applied on the host

Every figure is the best of three, warmed, and ends in a synchronise.  Evidence, not a unit test.

Under its own time limit:
    timeout -k 10 600 python profiles/probes/mix_probe.py 2048"""
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
    with open(os.path.join(ROOT, "profiles", "mix_probe.jsonl"), "a") as f:
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


def main(bits: int):
    import torch

    import paillier_halo2_amd as pz
    from oracle import cref
    from oracle import pyref as P
    from paillier_halo2_amd import mix

    cref.build()
    n, g = P.synth_paillier_inputs(bits, 0x3210)[:2]
    n2 = n * n
    Ln = -(-bits // 64)
    L = 2 * Ln
    lim = cref.int_to_limbs
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    nr = eng.ballot_steps_r(n)
    rng = random.Random(0x3211)
    n_w, g_w, three_w, n2_w = lim(n, Ln), lim(g, Ln), lim(3, Ln), lim(n2, L)
    for K in (1, 4, 64, 256, 1024):
        cts = [rng.randrange(n2) for _ in range(K)]
        rs = [rng.randrange(1, n) for _ in range(K)]
        perm = mix.random_permutation(K, rand=rng.randrange)
        sw = eng.mix_route(perm)
        c_w, r_w, zero_w = np.stack([lim(c, L) for c in cts]), np.stack([lim(r, Ln) for r in rs]), np.zeros((K, L), dtype=np.uint64)
        layers = eng.mix_layers(K)
        d_routes = torch.zeros((max(layers, 1), K, L), dtype=torch.int64, device="cuda")
        d_steps = torch.zeros((K, nr + 1, 4, L), dtype=torch.int64, device="cuda")
        d_ballot = torch.zeros((K, 2 + nr + 1, 4, L), dtype=torch.int64, device="cuda")
        whole = lambda: eng.paillier_mix_dev(Ln, n_w, c_w, sw, r_w, d_routes.data_ptr(), d_steps.data_ptr(), K * (nr + 1))
        route = lambda: eng.paillier_mix_dev(Ln, three_w, zero_w, sw, r_w, d_routes.data_ptr(), d_steps.data_ptr(), K * 5)
        chains = lambda: eng.paillier_ballot_dev(Ln, n_w, g_w, np.zeros(K, dtype=np.uint64), r_w, 1, d_ballot.data_ptr(), K * (2 + nr + 1))
        whole()
        mixed, t_whole = _timed(eng, whole)
        assert [cref.limbs_to_int(row) for row in mixed[:2]] == [cts[p] * pow(r, n, n2) % n2 for p, r in list(zip(perm, rs))[:2]]
        route()
        _, t_route = _timed(eng, route)
        chains()
        (rn, _), t_chains = _timed(eng, chains)

        def products():
            return [eng.mul_mod(L, c_w[perm[i]], rn[i], n2_w)[1] for i in range(K)]

        products()
        prod, t_prod = _timed(eng, products)
        assert np.array_equal(np.stack(prod), mixed)
        _emit({"probe": "k3", "bits": bits, "K": K, "layers": layers, "n_steps_r": nr, "mix_dev_ms": t_whole, "route_ms": t_route,
               "rerand_ms": t_whole - t_route, "parent_ms": t_chains + t_prod, "parent_chains_ms": t_chains, "parent_products_ms": t_prod})
        del d_routes, d_steps, d_ballot
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 2048))
