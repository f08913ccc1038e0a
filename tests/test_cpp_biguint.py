"""the host mirror's integers (paillier_halo2_amd/host/biguint.hpp) against Python integers, operation by operation, on the structured
catalogue of tests/k3_operands.py: limb counts 1, 2, 3, 64 and 128; equal operands, a - a, shifts and low_bits at 0, 63, 64 and 65;
division by 1, by itself and by a larger value; inverses with no unit and of zero.  tests/cpp/biguint_check.cpp is the driver.  CPU
only.  (gcd and mod_inverse divide bit by bit at every Euclidean step: at 64 and 128 limbs they run on operands whose chains are
short -- 1, 2, m - 1, (m + 1) / 2, a factor -- and on everything at 1, 2 and 3 limbs.)"""
import math
import os
import random
import subprocess

import pytest

from tests import k3_operands as K

HERE = os.path.dirname(os.path.abspath(__file__))
LIMBS = (1, 2, 3, 64, 128)
SHIFTS = (0, 1, 63, 64, 65, 127, 128)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("biguint") / "biguint_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", out, os.path.join(HERE, "cpp", "biguint_check.cpp")], check=True)
    return out


def _values(limbs):
    """structured values of up to `limbs` limbs: per top-limb length the modulus classes and the operand classes under the first"""
    out = [0, 1, 2, (1 << 64) - 1, 1 << 63]
    for tb in (1, 33, 64):
        ms = K.moduli(K.bits_of(limbs, tb))
        out += list(ms.values())
        m = ms["all_ones"]
        ops = K.operands(m, max(limbs, 2))
        out += [ops[k] for k in ("m-1", "m-2", "floor(m/2)", "isqrt", "isqrt+1", "ones", "alt64", "alt32_hi", "alt32_lo", "2^top") if k in ops]
    seen, uniq = set(), []
    for v in out:
        if v not in seen and v >> (64 * limbs) == 0:
            seen.add(v)
            uniq.append(v)
    return uniq


def cases():
    """[(line, expected output)]"""
    out = []
    h = lambda x: "%x" % x
    add = lambda op, a, b, third, want: out.append(("%s %s %s %s" % (op, h(a), h(b), third), want))
    thrown = lambda t: "throw:" + t
    for limbs in LIMBS:
        vals = _values(limbs)
        rng = random.Random(0x6d00 + limbs)
        big = limbs >= 64
        pairs = [(a, a) for a in vals] + [(a, vals[(i + 1) % len(vals)]) for i, a in enumerate(vals)] + \
                [(a, vals[(i * 7 + 3) % len(vals)]) for i, a in enumerate(vals)]
        pairs += [(rng.getrandbits(64 * limbs), rng.getrandbits(64 * limbs)) for _ in range(8)]
        for a, b in pairs:
            add("add", a, b, "", h(a + b))
            add("sub", a, b, "", h(a - b) if a >= b else thrown("range_error"))
            add("mul", a, b, "", h(a * b))
            add("lt", a, b, "", "%d %d %d" % (a < b, a == b, a != b))
        for a in vals:
            add("hex", a, 0, "", h(a))
            add("sub", a, a, "", "0")
            for s in SHIFTS + (64 * limbs - 1, 64 * limbs):
                add("shl", a, 0, s, h(a << s))
                add("shr", a, 0, s, h(a >> s))
                add("low_bits", a, 0, s, h(a & ((1 << s) - 1)))
            add("bits", a, 0, 63, "%d %d %d %d" % (a.bit_length(), a == 0, (a >> 63) & 1, -(-a.bit_length() // 64)))
            add("limbs", a, 0, limbs, h(a))
            if a >> 64:
                add("limbs", a, 0, -(-a.bit_length() // 64) - 1, thrown("range_error"))
            for w in (0, 1, 3, (1 << 63) + 1, (1 << 64) - 1):
                add("mul_small", a, w, "", h(a * w))
                add("divmod_small", a, w, "", "%x %x" % divmod(a, w) if w else thrown("domain_error"))
        # division: by 1, by itself, by a larger value, by zero, a double-length dividend by every modulus class
        nd = 6 if big else 12
        divs = [(a, 1) for a in vals[-nd:]] + [(a, a) for a in vals[-nd:]] + [(a, a + 1) for a in vals[-6:]] + [(vals[5], 0)]
        mods = [m for tb in (1, 64) for m in K.moduli(K.bits_of(limbs, tb)).values()]
        divs += [(a * b, m) for m in mods[: 4 if big else 16] for a, b in ((m - 1, m - 1), (m - 1, 1), (math.isqrt(m) + 1, math.isqrt(m) + 1))]
        divs += [(m * 3, m) for m in mods[:4]] + [(rng.getrandbits(128 * limbs), rng.getrandbits(64 * limbs) | 1) for _ in range(2 if big else 8)]
        for a, b in divs:
            add("divmod", a, b, "", " ".join(["%x %x" % divmod(a, b)] * 2) if b else thrown("domain_error"))
        add("divmod", 0, 0, "", thrown("domain_error"))
        # reduce_near: r < m 2^(k + 1) comes back reduced; r = m 2^(k + 1) does not
        for m in [x for x in mods if x > 1][:4]:
            for k in (0, 1, 8):
                for r in (0, m - 1, m, (m << (k + 1)) - 1, (m << k) + 1, K.alt64((m << k).bit_length() - 1)):
                    add("reduce_near", r, m, k, h(r % m))
                add("reduce_near", m << (k + 1), m, k, thrown("range_error"))
        add("reduce_near", 5, 0, 1, thrown("domain_error"))
        # gcd / mod_inverse
        odd = [m for m in mods if m & 1 and m > 2]
        if big:
            inv = [(x, m) for m in odd[:3] for x in (1, 2, m - 1, m - 2, (m + 1) // 2, 0)]
            p, q = K.mersenne_primes(6)
            n = p * q if limbs == 64 else p * q * ((1 << 4000) + 1)
            inv += [(p, n), (q, n), (0, n), (1, n), (n - 1, n), (n, n)]
            gcds = [(n, p), (p, n), (n, 0), (0, n), (n, n), (n - 1, n)]
        else:
            inv = [(x, m) for m in odd for x in _values(limbs)[:20]] + [(rng.getrandbits(64 * limbs), m) for m in odd[:4] for _ in range(4)]
            inv += [(3, 9), (6, 9), (0, 7), (7, 7), (8, 7), (1, 1), (5, 1)]
            gcds = [(a, b) for a, b in pairs[:40]] + [(0, 0), (0, 5), (5, 0), (12, 18)]
        for x, m in inv:
            ok = math.gcd(x % m, m) == 1
            add("mod_inverse", x, m, "", h(pow(x, -1, m) if m > 1 else 0) if ok else thrown("domain_error"))
        add("mod_inverse", 3, 0, "", thrown("domain_error"))
        for a, b in gcds:
            add("gcd", a, b, "", h(math.gcd(a, b)))
    out.append(("hex 00ff 0", "ff"))
    out.append(("hex ABCdef0123456789abcdef 0", "abcdef0123456789abcdef"))
    out.append(("hex 12g4 0", "throw:invalid_argument"))
    return out


def run_cases(exe):
    cs = cases()
    res = subprocess.run([exe], input="".join(line + "\n" for line, _ in cs), check=True, capture_output=True, text=True)
    got = res.stdout.splitlines()
    assert len(got) == len(cs)
    return cs, got


def test_biguint_equals_python_integers(exe):
    cs, got = run_cases(exe)
    bad = [(line[:160], g[:80], w[:80]) for (line, w), g in zip(cs, got) if g != w]
    assert not bad, bad[:5]
    ops = {line.split()[0] for line, _ in cs}
    assert ops == {"add", "sub", "mul", "shl", "shr", "low_bits", "divmod", "mul_small", "divmod_small", "reduce_near", "gcd", "mod_inverse", "lt",
                   "bits", "hex", "limbs"}
    assert sum(w.startswith("throw:") for _, w in cs) > 50 and len(cs) > 5000
