"""Writes tests/golden/paillier_keys.json: one prime pair (p, q) per key size the decryption tests use, from a seeded generator in
pure Python (Miller-Rabin, 40 seeded bases after trial division).  Every n = p q has exactly `bits` bits and gcd(n, phi(n)) = 1.
Run from the repository root: python tests/golden/make_paillier_keys.py"""
import json
import math
import os
import random

SIZES = (128, 264, 1024, 2048, 2112, 3072, 4096)
SMALL = [p for p in range(3, 2000, 2) if all(p % d for d in range(3, int(p ** 0.5) + 1, 2))]


def is_prime(n: int, rng: random.Random) -> bool:
    if n < 2 or n % 2 == 0:
        return n == 2
    for p in SMALL:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(40):
        x = pow(rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime(bits: int, rng: random.Random) -> int:
    while True:
        c = rng.getrandbits(bits) | (3 << (bits - 2)) | 1      # two top bits set: the product of two has exactly 2 * bits bits
        if is_prime(c, rng):
            return c


def main():
    keys = {}
    for bits in SIZES:
        rng = random.Random(0x9a11 + bits)
        while True:
            p, q = prime(bits // 2, rng), prime(bits - bits // 2, rng)
            n = p * q
            if p != q and n.bit_length() == bits and math.gcd(n, (p - 1) * (q - 1)) == 1:
                break
        keys[str(bits)] = {"p": hex(p), "q": hex(q)}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "paillier_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
