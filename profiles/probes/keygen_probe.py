"""Times the device prime generation:
    python keygen_probe.py mr             Miller-Rabin rounds per second of pz_bigint_is_prime_dev on a full batch (65536 random odd
                                          candidates, 2 rounds) at 8, 16, 24 and 32 limbs, beside (b) below
    python keygen_probe.py key            wall time of keys.generate_key at 2048 bits, plain and safe (best and mean of three keys each)
    python keygen_probe.py python [cap]   reference (a): the same two searches by the only generator the project had, the Python loop of
                                          tests/golden/make_paillier_keys.py (trial division, then Miller-Rabin by pow) on this host; the
                                          safe search stops after `cap` seconds (default 120) and then reports candidates per second
Reference (b): the kernel issues (8 E + 1) limbs v_mad_u64_u32 per lane and Montgomery product (E = 1 up to 16 limbs, 2 above; counted in
the ISA: 8 E for the two 64 x 64 products of a step and one for m) and a round is 2 x 64 limbs products, so a round of one candidate is
16 lanes x 128 limbs^2 (8 E + 1) lane-mads; over the issue rate libpz_probe measures live (bench.py's roofline_int peak) that is the
least time the multiplier could take, and mad_frac is that over the measured time.
Appends one JSON line per run to profiles/keygen_probe.jsonl (and prints it).  Every device figure ends in a synchronise; every result is
checked against Python integers first.  Evidence, not a unit test.

Each step under its own time limit, chained:
    timeout -k 10 240 python profiles/probes/keygen_probe.py mr && timeout -k 10 240 python profiles/probes/keygen_probe.py key && \\
    timeout -k 10 400 python profiles/probes/keygen_probe.py python 120"""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
BITS = 2048


def mr(eng, out):
    import torch
    from paillier_halo2_amd import probe
    from tests import prime_ref as R

    mad_peak = max(8192 * 256 * 1024 * 8 / (probe.ubench_mad_indep(0, 8192, 1024) * 1e-3) for _ in range(3))   # lane-mads per second
    out["mad_peak_tmads"] = mad_peak / 1e12
    count, rounds = 65536, 2
    rng = random.Random(0x7ea0)
    bases = np.array([rng.getrandbits(64) | 2 for _ in range(rounds)], dtype=np.uint64)
    for limbs in (8, 16, 24, 32):
        cands = np.frombuffer(rng.randbytes(count * limbs * 8), dtype=np.uint64).reshape(count, limbs).copy()
        cands[:, 0] |= 1
        cands[:, -1] |= 1 << 63
        cands[0] = R.words((1 << 127) - 1, limbs)                      # one prime among them: its flag is checked below
        d_c = torch.from_numpy(cands.astype(np.int64)).cuda()
        d_fl = torch.zeros(count, dtype=torch.uint8, device="cuda")
        d_w = torch.zeros(count, dtype=torch.int32, device="cuda")
        run = lambda: eng.is_prime_dev(limbs, count, d_c.data_ptr(), bases, d_fl.data_ptr(), d_w.data_ptr())
        run()
        eng.sync()
        fl = d_fl.cpu().numpy()
        ints = [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in cands[:64]]
        assert [int(f) for f in fl[:64]] == [R.mr_first_witness(c, bases.tolist())[0] for c in ints]
        best = None
        for _ in range(3):
            eng.sync()
            t0 = time.perf_counter()
            run()
            eng.sync()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        E = 1 if limbs <= 16 else 2
        mads = count * rounds * 16 * 128 * limbs * limbs * (8 * E + 1)
        out["limbs%d" % limbs] = {"ms": best * 1e3, "rounds_per_s": count * rounds / best, "passed": int(fl.sum()),
                                  "mad_bound_ms": mads / mad_peak * 1e3, "mad_frac": mads / mad_peak / best}


def key(eng, out):
    from paillier_halo2_amd import keys

    rng = random.Random(0x7ea1)
    for safe in (False, True):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            p, q = keys.generate_key(eng, BITS, safe=safe, rand=rng.getrandbits)
            times.append(time.perf_counter() - t0)
            assert (p * q).bit_length() == BITS and keys._is_prime(p) and keys._is_prime(q)
            assert not safe or (keys._is_prime((p - 1) // 2) and keys._is_prime((q - 1) // 2))
        out["safe_key_s" if safe else "plain_key_s"] = {"best": min(times), "mean": sum(times) / 3}


def python_reference(out, cap):
    """the fixture generator's loop (trial division by the odd primes below 2000, then Miller-Rabin by pow), seeded"""
    from paillier_halo2_amd import keys

    small = [p for p in range(3, 2000, 2) if all(p % d for d in range(3, int(p ** 0.5) + 1, 2))]
    rng = random.Random(0x7ea2)
    sieved = lambda c: all(c % p for p in small)
    t0 = time.perf_counter()
    for _ in range(2):
        while True:
            c = rng.getrandbits(BITS // 2) | (3 << (BITS // 2 - 2)) | 1
            if sieved(c) and keys._is_prime(c):
                break
    out["python_plain_key_s"] = time.perf_counter() - t0
    t0, tried, found = time.perf_counter(), 0, 0
    while found < 2 and time.perf_counter() - t0 < cap:
        c = rng.getrandbits(BITS // 2) | (3 << (BITS // 2 - 2)) | 3
        tried += 1
        if sieved(c) and sieved(c >> 1) and keys._is_prime(c >> 1) and keys._is_prime(c):
            found += 1
    dt = time.perf_counter() - t0
    out["python_safe"] = {"seconds": dt, "candidates": tried, "safe_primes_found": found, "finished": found == 2, "candidates_per_s": tried / dt}


def main(argv):
    out = {"probe": argv[0], "bits": BITS}
    if argv[0] == "python":
        python_reference(out, float(argv[1]) if len(argv) > 1 else 120.0)
    else:
        import paillier_halo2_amd as pz

        eng = pz.Engine(0)
        eng.bind_torch_stream()
        (mr if argv[0] == "mr" else key)(eng, out)
        eng.close()

    def rnd(v):
        return {k: rnd(x) for k, x in v.items()} if isinstance(v, dict) else float("%.4g" % v) if isinstance(v, float) else v

    line = json.dumps(rnd(out))
    print(line)
    with open(os.path.join(ROOT, "profiles", "keygen_probe.jsonl"), "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:] or ["mr"]))
