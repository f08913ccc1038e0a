"""Times the device modular inverse and the t-of-T combiner at 2048 bits:
    python shamir_probe.py inverse            pz_bigint_mod_inverse_dev for count in {1, 256, 4096} under a 2048-bit n
    python shamir_probe.py combine T t        pz_paillier_combine_t_dev for t of T trustees (the members T - t + 1 .. T) at K in {1, 64},
                                              and beside it pz_paillier_combine_dev at the same member count and K (the T-of-T combiner
                                              run on the same partials: its flags are set, its work is the same t - 1 products)
Appends one JSON line per run to profiles/shamir_probe.jsonl (and prints it).  Every figure is the best of three, warmed, and ends in a
synchronise; every result is checked against Python integers first.  Evidence, not a unit test.

Each GPU step under its own time limit, chained:
    timeout -k 10 120 python profiles/probes/shamir_probe.py inverse && timeout -k 10 120 python profiles/probes/shamir_probe.py combine 5 3 && \\
    timeout -k 10 120 python profiles/probes/shamir_probe.py combine 16 9 && timeout -k 10 300 python profiles/probes/shamir_probe.py combine 256 129
(the section's table; t = 129 of 256 is about 130 000 dependent mul_mods a launch)"""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
BITS = 2048


def _timed(eng, fn, reps=3):
    best = None
    for _ in range(reps):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def inverse(eng, out):
    import torch
    from oracle import cref
    from tests import decrypt_ref as DR

    p, q = DR.primes(BITS)
    n, Ln = p * q, BITS // 64
    lim = cref.int_to_limbs
    rng = random.Random(0x7d90)
    for count in (1, 256, 4096):
        xs = [rng.randrange(1, n) for _ in range(count)]
        d_x = torch.from_numpy(np.stack([lim(x, Ln) for x in xs]).astype(np.int64)).cuda()
        d_inv = torch.zeros((count, Ln), dtype=torch.int64, device="cuda")
        d_fl = torch.zeros(count, dtype=torch.uint8, device="cuda")
        run = lambda: eng.mod_inverse_dev(Ln, lim(n, Ln), count, d_x.data_ptr(), d_inv.data_ptr(), d_fl.data_ptr())
        run()
        eng.sync()
        got = d_inv.cpu().numpy().view(np.uint64)
        assert not d_fl.cpu().numpy().any() and all(cref.limbs_to_int(got[j]) == pow(xs[j], -1, n) for j in range(min(count, 64)))
        out["mod_inverse_dev_count%d_ms" % count] = _timed(eng, run)


def combine(eng, out, T, t):
    import torch
    from oracle import cref
    from paillier_halo2_amd import keys
    from tests import decrypt_ref as DR
    from tests import shamir_ref as SR

    p, q = DR.primes(BITS)
    rng = random.Random(0x7d91 + T)
    n, g, shares, mu2 = SR.deal(p, q, T, t, rng.randrange)
    n2, Ln = n * n, BITS // 64
    L = 2 * Ln
    lim = cref.int_to_limbs
    ids = list(range(T - t + 1, T + 1))
    mus = keys.lagrange_exponents(T, ids)
    out.update(trustees=T, threshold=t, exp_bits=max(abs(m).bit_length() for m in mus), set_bits=sum(bin(abs(m)).count("1") for m in mus))
    # K ciphertexts from one honest one by the homomorphism: c_j = c_0^(j + 1) encrypts (j + 1) m_0 and u_i(c_j) = u_i(c_0)^(j + 1)
    m0 = rng.randrange(n)
    c0 = SR.encrypt(n, g, m0, rng.randrange(1, n), pq=(p, q))
    u0 = [SR.partial(c0, shares[i - 1], n, pq=(p, q)) for i in ids]
    for K in (1, 64):
        parts = np.stack([np.stack([lim(pow(u, j + 1, n2), L) for j in range(K)]) for u in u0])
        d_parts = torch.from_numpy(parts.astype(np.int64)).cuda()
        d_m = torch.zeros((K, Ln), dtype=torch.int64, device="cuda")
        d_fl = torch.zeros(K, dtype=torch.uint8, device="cuda")
        run = lambda: eng.paillier_combine_t_dev(Ln, (n, mu2, T), ids, K, d_parts.data_ptr(), d_m.data_ptr(), d_fl.data_ptr())
        run()
        eng.sync()
        assert not d_fl.cpu().numpy().any()
        assert [cref.limbs_to_int(r) for r in d_m.cpu().numpy().view(np.uint64)] == [(j + 1) * m0 % n for j in range(K)]
        out["combine_t_dev_K%d_ms" % K] = _timed(eng, run)
        plain = lambda: eng.paillier_combine_dev(Ln, lim(n, Ln), lim(mu2, Ln), K, t, d_parts.data_ptr(), d_m.data_ptr(), d_fl.data_ptr())
        plain()
        out["combine_dev_same_members_K%d_ms" % K] = _timed(eng, plain)


def main(argv):
    import paillier_halo2_amd as pz
    from oracle import cref

    cref.build()
    eng = pz.Engine(0)
    eng.bind_torch_stream()
    out = {"probe": argv[0], "bits": BITS}
    if argv[0] == "inverse":
        inverse(eng, out)
    else:
        combine(eng, out, int(argv[1]), int(argv[2]))
    eng.close()
    out = {f: round(v, 3) if isinstance(v, float) else v for f, v in out.items()}
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, "profiles", "shamir_probe.jsonl"), "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:] or ["inverse"]))
