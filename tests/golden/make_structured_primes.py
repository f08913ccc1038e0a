"""Writes tests/golden/structured_primes.json: for k in {256, 512, 1024} the smallest c1 with 2^k - c1 prime, the next such c2, and
the smallest c_low with 2^(k-1) + c_low prime, by paillier_halo2_amd.keys._is_prime.  Deterministic, CPU only, a few seconds.
tests/k3_operands.py builds the structured-prime Paillier keys from it: primes that are one long run of ones (or of zeros) with a
short tail, so n, n^2 and lambda are runs too."""
import json
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


def main():
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
