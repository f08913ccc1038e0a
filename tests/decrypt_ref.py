"""Test-side restatement of decryption with randomness recovery and of the decrypt circuit (kind 5 / "decrypt"; DESIGN.md section
15.9), independent of the product: Python integers, the key fixtures of tests/golden/paillier_keys.json, oracle.pyref's encryption
and its uniform-shape cell stream.  The product must not import this module.

A key is (n, g, lam, d, mu, ginv): lam = lcm(p - 1, q - 1), d = n^-1 mod lam, mu = L(g^lam mod n^2)^-1 mod n, ginv = g^-1 mod n."""
import json
import math
import os
import random
from typing import List, Tuple

from oracle import pyref as P

KEY_BITS = (128, 264, 1024, 2048, 2112, 3072, 4096)


def primes(bits: int) -> Tuple[int, int]:
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paillier_keys.json")) as f:
        k = json.load(f)[str(bits)]
    return int(k["p"], 16), int(k["q"], 16)


def key(bits: int, standard_g: bool = True, seed: int = 0):
    p, q = primes(bits)
    n = p * q
    lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    assert n.bit_length() == bits and math.gcd(n, (p - 1) * (q - 1)) == 1
    g = n + 1
    if not standard_g:
        rng = random.Random(0x6e6 + bits + seed)
        while True:     # below n (g has n's limbs in the circuit), of an order n divides: all but ~1/p + 1/q of the residues
            g = rng.randrange(2, n)
            u = pow(g, lam, n * n)
            if math.gcd(g, n) == 1 and u % n == 1 and math.gcd(u // n, n) == 1:
                break
    x = pow(g, lam, n * n) // n
    return n, g, lam, pow(n, -1, lam), pow(x, -1, n), pow(g, -1, n)


def decrypt_ref(k, c: int) -> Tuple[int, int, int]:
    """-> (m, r, flag): flag 1 (and zeros) if c is no unit mod n"""
    n, g, lam, d, mu, ginv = k
    u = pow(c, lam, n * n)
    if u % n != 1:
        return 0, 0, 1
    m = (u // n) * mu % n
    r = pow(c % n * pow(ginv, m, n) % n, d, n)
    return m, r, 0


def messages(n: int, count: int, rng: random.Random) -> List[int]:
    """0, 1, n - 1, then random"""
    special = [0, 1, n - 1]
    return [special[i] if i < 3 else rng.randrange(n) for i in range(count)]


def encryptions(k, count: int, seed: int):
    """-> (ms, rs, cs): oracle.pyref.paillier_enc_native of `messages` under units r; the LAST one is encrypted with r + n (an r >= n:
    it must come back reduced), so rs holds what decryption returns"""
    n, g = k[0], k[1]
    rng = random.Random(seed)
    ms = messages(n, count, rng)
    rs, cs = [], []
    for i, m in enumerate(ms):
        while True:
            r = rng.randrange(1, n)
            if math.gcd(r, n) == 1:
                break
        cs.append(P.paillier_enc_native(n, g, m, r + n if i == count - 1 else r))
        rs.append(r)
    return ms, rs, cs


def statement(n: int, g: int, m: int, c: int, enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | g[Ln] | m[Ln] | c[2 Ln], little-endian limbs"""
    Ln = enc_bits // limb_bits
    return (P.decompose_biguint(n, Ln, limb_bits) + P.decompose_biguint(g, Ln, limb_bits) + P.decompose_biguint(m, Ln, limb_bits) +
            P.decompose_biguint(c, 2 * Ln, limb_bits))


def exposed_cells(n: int, g: int, m: int, r: int, c: int, enc_bits: int, limb_bits: int, lb: int) -> Tuple[List[int], List[int]]:
    """-> (stream indices of the exposed cells, the advice stream) from oracle.pyref's uniform-shape stream: the limb cells at the head
    of assign_integer(n), (g), (m) -- the third -- and of the last assign_integer, res"""
    Ln = enc_bits // limb_bits
    adv, _, seg = P.expand_uniform_circuit_cells(n, g, m, r, c, enc_bits, limb_bits, lb)
    assert seg["satisfied"]
    cells = [seg[name][0] + j for name in ("assign_n", "assign_g", "assign_x") for j in range(Ln)]
    return cells + [seg["assign_res"][0] + j for j in range(2 * Ln)], adv
