"""Writes tests/golden/structured_primes.json: for k in {256, 512, 1024} the smallest c1 with 2^k - c1 prime, the next such c2, and
the smallest c_low with 2^(k-1) + c_low prime, by paillier_halo2_amd.keys._is_prime.  Deterministic, CPU only, a few seconds.
tests/k3_operands.py builds the structured-prime Paillier keys from it: primes that are one long run of ones (or of zeros) with a
short tail, so n, n^2 and lambda are runs too.

Also writes tests/golden/structured_prime_patterns.json for tests/prime_operands.py (a file of its own: tests/test_k3_operands.py reads
every key of the first file as a bit length):
  "patterns": for every limb count 1 .. 32 and every modulus pattern at full width, [limbs, pattern, k, sign] with the smallest k >= 0
              such that pattern + sign 2 k is prime and still has 64 limbs bits; primality here is Miller-Rabin over Python integers with
              the first 40 primes as bases
  "proth":    [s, k, z]: the smallest odd k with k 2^s + 1 prime and the smallest z with Jacobi symbol (z / c) = -1
and runs the two searches whose results tests/prime_operands.py lists: composites c with a base a such that a^(c-1) = -1 mod c (every
base below 2^12, the per-prime-power criterion below 2^20), and the (a, b, c) triples that reach the look-ahead's carry out and long
carry ripples in the model (printed as the lines of SEARCHED).  Deterministic, CPU only, a few minutes."""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from paillier_halo2_amd.keys import _is_prime  # noqa: E402


def below(k: int, start: int) -> int:
    c = start
    while not _is_prime((1 << k) - c):
        c += 1
    return c


def above(k: int) -> int:
    c = 1
    while not _is_prime((1 << k) + c):
        c += 1
    return c


BASES40 = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131, 137,
           139, 149, 151, 157, 163, 167, 173)
PROTH_S = (127, 128, 129, 1023, 1024, 1025, 1983, 1984, 1985)


def is_prime40(c: int) -> bool:
    from tests import prime_ref

    if c < 2:
        return False
    for p in prime_ref.SIEVE_PRIMES[:300] + [2]:
        if c % p == 0:
            return c == p
    return pow(2, c - 1, c) == 1 and prime_ref.mr_first_witness(c, BASES40)[0] == 1


def patterns():
    from tests import prime_operands as PO

    out = []
    for limbs in PO.LIMBS_ALL:
        ms = PO.moduli(limbs, 64)
        for name in PO.PATTERNS:
            if name not in ms:
                continue
            sign = 1 if name == "pow2_plus1" else -1
            k = 0
            while not is_prime40(ms[name] + sign * 2 * k):
                k += 1
            assert (ms[name] + sign * 2 * k).bit_length() == 64 * limbs
            out.append([limbs, name, k, sign])
        print("patterns", limbs, out[-len(PO.PATTERNS):], flush=True)
    return out


def proth():
    from tests import prime_operands as PO

    out = []
    for s in PROTH_S:
        k = 1
        while not is_prime40(k * 2 ** s + 1):
            k += 2
        c = k * 2 ** s + 1
        z = 2
        while PO.jacobi(z, c) != -1:
            z += 1
        out.append([s, k, z])
    print("proth", out, flush=True)
    return out


def minus_one_search():
    """odd composites c with a base a such that a^(c-1) = -1 mod c: literally below 2^12, and below 2^20 by the Chinese remainder
    theorem -- x^m = -1 is solvable modulo p^e (a cyclic group of order phi) iff phi / gcd(m, phi) is even"""
    brute = [(c, a) for c in range(9, 1 << 12, 2) for a in range(2, c - 1) if pow(a, c - 1, c) == c - 1]
    limit = 1 << 20
    spf = list(range(limit))
    for p in range(2, 1 << 10):
        if spf[p] == p:
            for q in range(p * p, limit, p):
                if spf[q] == q:
                    spf[q] = p
    crit = []
    for c in range(9, limit, 2):
        if spf[c] == c:
            continue
        x, ok = c, True
        while x > 1 and ok:
            p, pe = spf[x], 1
            while x % p == 0:
                x, pe = x // p, pe * p
            phi = pe // p * (p - 1)
            g = math.gcd(c - 1, phi)
            ok = (phi // g) % 2 == 0
        if ok:
            crit.append(c)
    print("a^(c-1) = -1 mod c: brute force below 2^12", brute, "; criterion below 2^20", crit, flush=True)
    return brute, crit


def searched():
    """the first seed per goal: SEARCHED's lines"""
    from tests import prime_operands as PO

    lines = []
    for L in (16, 32, 8, 17):
        E, found = PO.capacity(L), {}
        for cls in ("R-3", "all_ones", "pow2_plus1", "minus_2_64_plus1"):
            c = PO.pattern(cls, L)
            for tg in ((1, 0), (3, 0), (4, 0), (-1, 0), (-2, 0), (1, 64 * (L - 1)), (1, 64 * (L // 2)), (5, 64 * (L - 1)), (1, 64 * E * 3)):
                if tg[0] << tg[1] >= c:
                    continue
                for seed in range(60):
                    s = PO.mont_mul_model(*PO.searched_triple(L, cls, seed, tg), L)
                    goals = {"out": s.out == 1, "out without a ripple": s.out == 1 and s.res_run == 0,
                             "resolve ripple to lane 15": s.res_run >= 3 and s.res_start + s.res_run == 16,
                             "resolve ripple inside": s.res_run >= 3 and s.res_start >= 4 and s.res_start + s.res_run < 16,
                             "resolve ripple": s.res_run >= 3,
                             "borrow ripple to lane 15": s.sub_run >= 3 and s.sub_start + s.sub_run == 16, "borrow ripple": s.sub_run >= 3}
                    for g, hit in goals.items():
                        if hit and g not in found:
                            found[g] = (L, cls, seed, tg, PO.searched_state(s))
        seen = []
        for g, (L_, cls, seed, tg, st) in found.items():
            if (cls, seed, tg) not in seen:
                seen.append((cls, seed, tg))
                lines.append("    (%d, %r, %d, %r, %r),   # %s" % (L_, cls, seed, tg, st, g))
    print("\n".join(lines), flush=True)
    return lines


def main():
    if "--searches" in sys.argv:
        minus_one_search()
        searched()
        return
    with open(os.path.join(HERE, "structured_prime_patterns.json"), "w") as f:
        json.dump({"patterns": patterns(), "proth": proth()}, f, separators=(",", ":"))
        f.write("\n")
    out = {}
    for k in (256, 512, 1024):
        c1 = below(k, 1)
        out[str(k)] = {"c1": c1, "c2": below(k, c1 + 1), "c_low": above(k - 1)}
    with open(os.path.join(HERE, "structured_primes.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
