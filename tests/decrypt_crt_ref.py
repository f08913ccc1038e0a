"""Test-side restatement of decryption by the CRT, independent of the product: Python integers over the
fixture primes of tests/golden/paillier_keys.json, and a catalogue of structured ciphertexts per key.  The product must not import
this module.

Per side P in {p, q}: u_P = (c mod P^2)^(P-1) mod P^2; c is a unit mod P iff u_P = 1 (mod P); m_P = ((u_P - 1) / P) h_P mod P with
h_P = (L_P(g^(P-1) mod P^2))^-1 mod P.  Garner: m = m_q + q (((m_p - m_q) mod p) qinv mod p).  The randomness: e_P = m mod (P - 1),
y_P = (c mod P) (ginv mod P)^e_P mod P, r_P = y_P^(d mod (P-1)) mod P, and the same Garner step."""
import functools
import math
import random
from typing import Dict, List, Tuple

from oracle import pyref as P
from tests import decrypt_ref as DR

FLAG_NOT_UNIT, FLAG_RANGE = 1, 2

key = functools.lru_cache(maxsize=None)(DR.key)      # DR.key(bits, standard_g), computed once: a general g costs a search with powers


@functools.lru_cache(maxsize=None)
def crt_key(bits: int, standard_g: bool = True, swap: bool = False) -> Dict[str, int]:
    """the values a CRT handle derives, from the fixture primes (swap: q in p's place) and DR.key's n, g, d"""
    n, g, lam, d, mu, ginv = key(bits, standard_g)
    p, q = DR.primes(bits)
    if swap:
        p, q = q, p
    k = {"n": n, "g": g, "d": d, "p": p, "q": q, "qinv": pow(q % p, p - 2, p)}
    for name, pr in (("p", p), ("q", q)):
        x = (pow(g % (pr * pr), pr - 1, pr * pr) - 1) // pr % pr
        k["h_" + name] = pow(x, pr - 2, pr)
        k["d_" + name] = d % (pr - 1)
        k["ginv_" + name] = ginv % pr
        assert x * k["h_" + name] % pr == 1
    assert q * k["qinv"] % p == 1
    return k


def garner(k: Dict[str, int], a_p: int, a_q: int) -> int:
    p, q = k["p"], k["q"]
    return a_q + q * ((a_p - a_q) % p * k["qinv"] % p)


def garner_sign(p: int, q: int, v: int) -> int:
    """the sign of Garner's difference v_p - (v_q mod p) before p is added back: -1 is a borrow"""
    a, b = v % p, v % q % p
    return (a > b) - (a < b)


def decrypt_crt_ref(k: Dict[str, int], c: int) -> Tuple[int, int, int]:
    """-> (m, r, flags): bit 0 (and zeros) if p | c or q | c, bit 1 (and zeros) if c >= n^2"""
    n = k["n"]
    if c >= n * n:
        return 0, 0, FLAG_RANGE
    ms, cs = {}, {}
    for name in ("p", "q"):
        pr = k[name]
        u = pow(c % (pr * pr), pr - 1, pr * pr)
        if u % pr != 1:
            return 0, 0, FLAG_NOT_UNIT
        ms[name] = (u - 1) // pr * k["h_" + name] % pr
        cs[name] = c % pr
    m = garner(k, ms["p"], ms["q"])
    rs = {}
    for name in ("p", "q"):
        pr = k[name]
        y = cs[name] * pow(k["ginv_" + name], m % (pr - 1), pr) % pr
        rs[name] = pow(y, k["d_" + name], pr)
    return m, garner(k, rs["p"], rs["q"]), 0


def _unit(n: int, rng: random.Random) -> int:
    while True:
        r = rng.randrange(2, n)
        if math.gcd(r, n) == 1:
            return r


_CATALOGUE = {}
NON_UNITS = ("p*k", "q", "0")


def catalogue(bits: int, standard_g: bool) -> List[Tuple[str, int, int, int]]:
    """-> [(label, c, m, r)] with (m, r) what decryption returns (zeros for the non-units and for n^2); computed once per key.
    NON_UNITS names the entries that p or q divides."""
    which = (bits, standard_g)
    if which in _CATALOGUE:
        return _CATALOGUE[which]
    n, g = key(bits, standard_g)[:2]
    p, q = DR.primes(bits)
    rng = random.Random(0xc47 + bits + standard_g)
    enc = lambda m, r: P.paillier_enc_native(n, g, m, r)
    out = []
    small = rng.randrange(2, min(p, q))
    for label, m in (("m=0", 0), ("m=1", 1), ("m=n-1", n - 1), ("m=p", p), ("m=q", q), ("m<min(p,q)", small)):
        r = _unit(n, rng)
        out.append((label, enc(m, r), m, r))
    for label, want in (("m_p<m_q", -1), ("m_p>m_q", 1)):
        while True:
            m = rng.randrange(n)
            if garner_sign(p, q, m) == want:
                break
        # the randomness goes the other way, so each entry borrows in exactly one of its two Garner steps
        while True:
            r = _unit(n, rng)
            if garner_sign(p, q, r) == -want:
                break
        out.append((label, enc(m, r), m, r))
    m = rng.randrange(n)
    out.append(("r=1", enc(m, 1), m, 1))
    m, r = rng.randrange(n), _unit(n, rng)
    out.append(("r+n", enc(m, r + n), m, r))
    out.append(("p*k", p * 0x1234567, 0, 0))
    out.append(("q", q, 0, 0))
    out.append(("0", 0, 0, 0))
    c = n * n - 1
    out.append(("n^2-1", c) + DR.decrypt_ref(key(bits, standard_g), c)[:2])
    out.append(("n^2", n * n, 0, 0))
    _CATALOGUE[which] = out
    return out
