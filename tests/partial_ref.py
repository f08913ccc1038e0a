"""Test-side restatement of T-of-T threshold decryption (circuit kind 7 / "partial"), independent of the
product: the scheme in Python integers (shares of theta = lambda (lambda^-1 mod n), partial decryptions u = (c^2)^theta_i, the
combiner), one trustee's trace h = v^theta, u_j = (c_j^2)^theta mod n^2 by oracle.pyref.pow_mod_uniform_trace, and the cell stream
composed from oracle.pyref's per-operation emitters with its gate mask from the gate_offsets_* functions.  The product must not import
this module.

Record order: the K squaring records (c_j, c_j, q, s_j), then chain i (0: the base v; j >= 1: s_j) at K + i 2 e_bits: bit t is
(acc, sq, q, r) then (sq, sq, q, sq')."""
import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from oracle import pyref as P
from tests.tally_ref import check_columns, place  # noqa: F401  (re-exported: the tests take them from here)

R = P.FR_R

# two 64-bit safe primes (p and (p - 1) / 2 both prime): a 128-bit n
SAFE_P, SAFE_Q = 0xA4E4E25A2BF9133F, 0xF6CC057211D86F37


# ------------------------------------------------------------------------------------------------ the scheme
def theta_of(p: int, q: int) -> int:
    n = p * q
    lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    return lam * pow(lam, -1, n)


def split(theta: int, N: int, trustees: int, rand) -> List[int]:
    """theta_1 .. theta_{T-1} = rand(N) each, theta_T = (theta - their sum) mod N"""
    shares = [rand(N) for _ in range(trustees - 1)]
    return shares + [(theta - sum(shares)) % N]


def mu2_of(n: int, g: int, theta: int) -> int:
    a = (pow(g, theta, n * n) - 1) // n
    return pow(2 * a, -1, n)


def partial(c: int, share: int, n: int) -> int:
    return pow(c * c % (n * n), share, n * n)


def combine(partials: Sequence[int], n: int, mu2: int):
    """-> (m, flag bit 0)"""
    U = 1
    for u in partials:
        U = U * u % (n * n)
    if U % n != 1:
        return 0, 1
    return (U - 1) // n * mu2 % n, 0


# ------------------------------------------------------------------------------------------------ one trustee's trace
class Trace(NamedTuple):
    h: int
    us: List[int]
    squares: List[P.Step]          # K records (c_j, c_j, q, s_j)
    chains: List[List[P.Step]]     # K + 1 chains of 2 e_bits steps
    exponents: List[int]           # what each chain was run with
    bases: List[int]               # each chain's first sq
    cts: List[int]                 # what each squaring block multiplied
    results: List[int]             # what each assert_equal_fresh compares with h / u_j


def partial_trace(n: int, v: int, theta: int, cts: Sequence[int], e_bits: int, forge=None) -> Trace:
    """forge, everything downstream of it recomputed consistently (the soundness negatives):
      ('exp', i, theta')  chain i runs with theta' while assign_integer(theta) keeps theta
      ('base', delta)     chain 0's first sq is v + delta
      ('ct', j, delta)    squaring block j (1 .. K) multiplies c_j + delta by itself
      ('sq', j, delta)    chain j's first sq is s_j + delta
      ('res', i, delta)   the assert_equal_fresh of chain i compares its result + delta"""
    n2 = n * n
    kind = forge[0] if forge is not None else None
    squares, chains, exps, bases, used, results = [], [], [], [], [], []
    for i in range(len(cts) + 1):
        e = forge[2] if kind == "exp" and forge[1] == i else theta
        if i == 0:
            base = v + (forge[1] if kind == "base" else 0)
        else:
            c = cts[i - 1] + (forge[2] if kind == "ct" and forge[1] == i else 0)
            st = P.mul_mod_step(c, c, n2)
            squares.append(st)
            used.append(c)
            base = st[3] + (forge[2] if kind == "sq" and forge[1] == i else 0)
        power, steps = P.pow_mod_uniform_trace(base, e, e_bits, n2)
        assert len(steps) == 2 * e_bits
        chains.append(steps)
        exps.append(e)
        bases.append(base)
        results.append(power + (forge[2] if kind == "res" and forge[1] == i else 0))
    return Trace(results[0], results[1:], squares, chains, exps, bases, used, results)


def records(trace: Trace) -> List[P.Step]:
    """the records in pz_paillier_partial's order"""
    out = list(trace.squares)
    for ch in trace.chains:
        out += list(ch)
    return out


def n_records(count: int, e_bits: int) -> int:
    return count + (count + 1) * 2 * e_bits


# ------------------------------------------------------------------------------------------------ the circuit
def _pow_cells(put, steps, e: int, n2: int, L: int, limb_bits: int, lb: int):
    """pow_mod(base, e) with e an assign_integer of L limbs, as kind 2 emits it: [1, 0], then per limb num_to_bits(limb, limb_bits) and
    that limb's blocks of mul_mod(acc, sq), limb-wise select, square_mod(sq)"""
    put("chains", [1, 0])
    el = P.decompose_biguint(e, L, limb_bits)
    for li in range(L):
        nb_cells, bits = P._num_to_bits_cells(el[li], limb_bits)
        put("chains", nb_cells)
        for bi in range(limb_bits):
            i = li * limb_bits + bi
            st_mul, st_sq = steps[2 * i], steps[2 * i + 1]
            put("chains", *P.expand_mul_mod_cells(*st_mul, n2, L, lb, limb_bits))
            acc_l, mul_l = P.decompose_biguint(st_mul[0], L, limb_bits), P.decompose_biguint(st_mul[3], L, limb_bits)
            for t in range(L):
                put("chains", P._select_cells(mul_l[t], acc_l[t], bits[bi]))
            put("chains", *P.expand_mul_mod_cells(*st_sq, n2, L, lb, limb_bits))


def partial_cells(n: int, v: int, theta: int, cts: Sequence[int], h: int, us: Sequence[int], enc_bits: int, limb_bits: int, lb: int,
                  trace: Optional[Trace] = None):
    """the stream: assign n, v, theta, c_1 .. c_K; square + refresh once, load_zero; pow_mod(v, theta); per j mul_mod(c_j, c_j) and
    pow_mod(s_j, theta); assign h + assert_equal_fresh; per j assign u_j + assert_equal_fresh.  The in-circuit exponent has 2 enc_bits
    bits.  trace = partial_trace's result to expand (default: the honest one); the assign_integer cells always hold v, theta and cts.
    -> (advice cells, lookup cells, {name: (advice offset, lookup offset)}) as canonical integers"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    n2 = n * n
    K = len(cts)
    if trace is None:
        trace = partial_trace(n, v, theta, cts, 2 * enc_bits)
    assert len(us) == K and len(trace.chains) == K + 1
    adv: List[int] = []
    lk: List[int] = []
    seg = {}

    def put(name, a, l=()):
        seg.setdefault(name, (len(adv), len(lk)))
        adv.extend(a)
        lk.extend(l)

    put("assign_n", *P.expand_assign_cells(n, Ln, limb_bits, lb))
    put("assign_v", *P.expand_assign_cells(v, L, limb_bits, lb))
    put("assign_theta", *P.expand_assign_cells(theta, L, limb_bits, lb))
    for c in cts:
        put("assign_cts", *P.expand_assign_cells(c, L, limb_bits, lb))
    nl = P.decompose_biguint(n, Ln, limb_bits)
    sq_cells, prod = P._mul_cells(nl, nl, 2 * Ln - 1)
    put("square", sq_cells)
    inc = P.refresh_aux(limb_bits, Ln, Ln)
    assert len(inc) == L
    r_adv, r_lk, fresh = P.expand_refresh_cells(prod, inc, limb_bits, lb)
    assert P.get_biguint(fresh, limb_bits) == n2
    put("refresh", r_adv, r_lk)
    put("load_zero", [0])
    for i in range(K + 1):
        if i:
            put("chains", *P.expand_mul_mod_cells(*trace.squares[i - 1], n2, L, lb, limb_bits))
        _pow_cells(put, trace.chains[i], trace.exponents[i], n2, L, limb_bits, lb)
    ok = True
    for got, want in zip(trace.results, [h] + list(us)):
        put("results", *P.expand_assign_cells(want, L, limb_bits, lb))
        ae, bit = P.expand_assert_equal_fresh_cells(P.decompose_biguint(got, L, limb_bits), P.decompose_biguint(want, L, limb_bits))
        put("results", ae)
        ok = ok and bool(bit)
    seg["end"] = (len(adv), len(lk))
    seg["satisfied"] = ok
    return [x % R for x in adv], [x % R for x in lk], seg


def partial_gate_mask(count: int, enc_bits: int, limb_bits: int, lb: int) -> np.ndarray:
    """uint8 selector over the advice stream (1 where a gate window starts), from the gate_offsets_* functions"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    W = limb_bits

    def mask(part):
        g, n = part
        m = np.zeros(n, dtype=np.uint8)
        m[np.asarray(g, dtype=np.int64)] = 1
        return m

    narrow = mask(P.gate_offsets_assign(Ln, limb_bits, lb))
    wide = mask(P.gate_offsets_assign(L, limb_bits, lb))
    mm = mask(P.gate_offsets_mul_mod(L, lb, limb_bits))
    parts = [narrow] + [wide] * (2 + count)
    parts.append(mask(P.gate_offsets_square(Ln)))
    parts.append(mask(P.gate_offsets_refresh(P.refresh_aux(limb_bits, Ln, Ln), limb_bits, lb)))
    parts.append(np.zeros(1, dtype=np.uint8))                            # load_zero
    two = np.zeros(2, dtype=np.uint8)
    ntb = mask(([3 * i for i in range(W - 1)] + [1 + 3 * (W - 1) + 4 * i for i in range(W)], 7 * W - 2))
    sel = mask(([8 * t + o for t in range(L) for o in (0, 4)], 8 * L))
    chain = np.concatenate([two] + [np.concatenate([ntb] + [mm, sel, mm] * W)] * L)
    parts.append(chain)
    parts += [mm, chain] * count
    parts += [wide, mask(P.gate_offsets_assert_equal(L))] * (count + 1)
    return np.concatenate(parts)


def statement(n: int, v: int, h: int, cts: Sequence[int], us: Sequence[int], enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | v[2 Ln] | h[2 Ln] | c_1[2 Ln] | u_1[2 Ln] | .. | c_K | u_K, little-endian limbs"""
    Ln = enc_bits // limb_bits
    assert len(cts) == len(us)
    out = P.decompose_biguint(n, Ln, limb_bits) + P.decompose_biguint(v, 2 * Ln, limb_bits) + P.decompose_biguint(h, 2 * Ln, limb_bits)
    for c, u in zip(cts, us):
        out += P.decompose_biguint(c, 2 * Ln, limb_bits) + P.decompose_biguint(u, 2 * Ln, limb_bits)
    return out
