"""Test-side restatement of the short-randomness ballot (circuit kind 9 / "sballot"), independent of the
product: the scheme in Python integers (hs = (-x^2 mod n)^n mod n^2, c = g^m hs^s mod n^2, decryption with the recovered randomness),
the trace of K ciphertexts under one key -- per ciphertext oracle.pyref.pow_mod_uniform_trace over b message bits on the base g, the
same over s_bits bits of s_i on the base hs, and one mul_mod_step -- and the cell stream composed from oracle.pyref's per-operation
emitters with its gate mask from the gate_offsets_* functions.  Python integers throughout.  The product must not import this module.

Record order: ciphertext-major, 2 b + 2 s_bits + 1 per entry: the g-chain's 2 b records (bit j: (acc, sq, q, r) then (sq, sq, q, sq')),
the hs-chain's 2 s_bits in the same form, the final (gm, hss, q, c)."""
import math
from typing import List, NamedTuple, Sequence

import numpy as np

from oracle import pyref as P
from tests.tally_ref import check_columns, place  # noqa: F401  (re-exported: the tests take them from here)

R = P.FR_R

# two 64-bit safe primes (both 3 mod 4): a 128-bit n
SAFE_P, SAFE_Q = 0xA4E4E25A2BF9133F, 0xF6CC057211D86F37


# ------------------------------------------------------------------------------------------------ the scheme
def djn_h(n: int, x: int) -> int:
    assert math.gcd(x, n) == 1
    return (-x * x) % n


def djn_hs(n: int, x: int) -> int:
    return pow(djn_h(n, x), n, n * n)


def encrypt(n: int, g: int, hs: int, m: int, s: int) -> int:
    return pow(g, m, n * n) * pow(hs, s, n * n) % (n * n)


def decrypt(p: int, q: int, g: int, c: int):
    """-> (m, r) with c = g^m r^n mod n^2, r in [0, n)"""
    n = p * q
    n2 = n * n
    lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    lf = lambda u: (u - 1) // n
    m = lf(pow(c, lam, n2)) * pow(lf(pow(g, lam, n2)), -1, n) % n
    rn = c * pow(g, -m, n2) % n2          # r^n mod n^2
    return m, pow(rn % n, pow(n, -1, lam), n)


# ------------------------------------------------------------------------------------------------ the trace
class Trace(NamedTuple):
    cts: List[int]                 # what each entry's final block leaves
    g_chains: List[List[P.Step]]   # 2 b steps each
    s_chains: List[List[P.Step]]   # 2 s_bits steps each
    finals: List[P.Step]
    m_exps: List[int]              # what each g-chain was run with
    s_exps: List[int]              # what each hs-chain was run with
    total: int                     # the last cell of the sum (K = 1: unused, the message)


def per_entry(m_bits: int, s_bits: int) -> int:
    return 2 * m_bits + 2 * s_bits + 1


def sballot_trace(n: int, g: int, hs: int, ms: Sequence[int], ss: Sequence[int], m_bits: int, s_bits: int, forge=None) -> Trace:
    """forge, everything downstream of it recomputed consistently (the soundness negatives):
      ('s', i, s')        hs-chain i runs with s' while assign_integer(s_i) keeps s_i
      ('base', i, delta)  hs-chain i's first sq is hs + delta
      ('msg', i, m')      g-chain i runs with m' while the load_witness cell keeps m_i
      ('g', i, delta)     g-chain i's first sq is g + delta
      ('final', i, delta) the final block's second operand is hss_i + delta
      ('sum', delta)      the last sum cell is S + delta"""
    n2 = n * n
    assert len(ms) == len(ss) >= 1
    t = Trace([], [], [], [], [], [], sum(ms) + (forge[1] if forge is not None and forge[0] == "sum" else 0))
    for i, (m, s) in enumerate(zip(ms, ss)):
        hit = lambda name: forge is not None and forge[0] == name and forge[1] == i
        me = forge[2] if hit("msg") else m
        se = forge[2] if hit("s") else s
        gm, sg = P.pow_mod_uniform_trace(g + (forge[2] if hit("g") else 0), me, m_bits, n2)
        hss, sh = P.pow_mod_uniform_trace(hs + (forge[2] if hit("base") else 0), se, s_bits, n2)
        assert len(sg) == 2 * m_bits and len(sh) == 2 * s_bits
        fin = P.mul_mod_step(gm, hss + (forge[2] if hit("final") else 0), n2)
        t.cts.append(fin[3])
        t.g_chains.append(sg)
        t.s_chains.append(sh)
        t.finals.append(fin)
        t.m_exps.append(me)
        t.s_exps.append(se)
    return t


def records(trace: Trace) -> List[P.Step]:
    """the records in pz_paillier_sballot's order"""
    out: List[P.Step] = []
    for sg, sh, fin in zip(trace.g_chains, trace.s_chains, trace.finals):
        out += list(sg) + list(sh) + [fin]
    return out


# ------------------------------------------------------------------------------------------------ the circuit
def sballot_cells(n: int, g: int, hs: int, ms: Sequence[int], ss: Sequence[int], res: Sequence[int], m_bits: int, s_limbs: int,
                  enc_bits: int, limb_bits: int, lb: int, trace: Trace = None):
    """the stream: assign n, g; assign hs at full width; load_witness(m_1 .. m_K); for K >= 2 FlexGate::sum of them; assign s_1 .. s_K
    (s_limbs limbs each); square + refresh once, load_zero; per ciphertext pow_mod(g_ext, m_i) over b bits as kind 6, pow_mod(hs, s_i)
    as kind 7 emits a chain ([1, 0], then per limb of s_i num_to_bits and that limb's blocks) and mul_mod; per ciphertext assign res_i
    and assert_equal_fresh(c_i, res_i).
    trace = sballot_trace's result to expand (default: the honest one).  The load_witness cells, the sum's operands and the
    assign_integer(s_i) always hold `ms` and `ss`; a chain's num_to_bits holds the exponent its records were run with.
    -> (advice cells, lookup cells, {name: (advice offset, lookup offset)}) as canonical integers"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    n2 = n * n
    K = len(ms)
    s_bits = s_limbs * limb_bits
    if trace is None:
        trace = sballot_trace(n, g, hs, ms, ss, m_bits, s_bits)
    assert len(trace.cts) == len(ss) == len(res) == K
    adv: List[int] = []
    lk: List[int] = []
    seg = {}

    def put(name, a, l=()):
        seg.setdefault(name, (len(adv), len(lk)))
        adv.extend(a)
        lk.extend(l)

    put("assign_n", *P.expand_assign_cells(n, Ln, limb_bits, lb))
    put("assign_g", *P.expand_assign_cells(g, Ln, limb_bits, lb))
    put("assign_hs", *P.expand_assign_cells(hs, L, limb_bits, lb))
    put("messages", [int(m) for m in ms])
    if K >= 2:
        cells, s = [int(ms[0])], int(ms[0])
        for i in range(1, K):
            s += int(ms[i])
            cells += [1, int(ms[i]), s]
        cells[-1] = trace.total
        assert len(cells) == 1 + 3 * (K - 1)
        put("sum", cells)
    for s in ss:
        put("assign_ss", *P.expand_assign_cells(s, s_limbs, limb_bits, lb))
    nl = P.decompose_biguint(n, Ln, limb_bits)
    sq_cells, prod = P._mul_cells(nl, nl, 2 * Ln - 1)
    put("square", sq_cells)
    inc = P.refresh_aux(limb_bits, Ln, Ln)
    assert len(inc) == L
    r_adv, r_lk, fresh = P.expand_refresh_cells(prod, inc, limb_bits, lb)
    assert P.get_biguint(fresh, limb_bits) == n2
    put("refresh", r_adv, r_lk)
    put("load_zero", [0])

    def bit_blocks(steps, bits, first):
        for j, bit in enumerate(bits):
            st_mul, st_sq = steps[2 * (first + j)], steps[2 * (first + j) + 1]
            put("entries", *P.expand_mul_mod_cells(*st_mul, n2, L, lb, limb_bits))
            acc_l, mul_l = P.decompose_biguint(st_mul[0], L, limb_bits), P.decompose_biguint(st_mul[3], L, limb_bits)
            for t in range(L):
                put("entries", P._select_cells(mul_l[t], acc_l[t], bit))
            put("entries", *P.expand_mul_mod_cells(*st_sq, n2, L, lb, limb_bits))

    for sg, sh, fin, me, se in zip(trace.g_chains, trace.s_chains, trace.finals, trace.m_exps, trace.s_exps):
        put("entries", [1, 0])
        nb_cells, bits = P._num_to_bits_cells(me, m_bits)
        assert len(nb_cells) == 7 * m_bits - 2
        put("entries", nb_cells)
        bit_blocks(sg, bits, 0)
        put("entries", [1, 0])
        sl = P.decompose_biguint(se, s_limbs, limb_bits)
        for li in range(s_limbs):
            nb_cells, bits = P._num_to_bits_cells(sl[li], limb_bits)
            put("entries", nb_cells)
            bit_blocks(sh, bits, li * limb_bits)
        put("entries", *P.expand_mul_mod_cells(*fin, n2, L, lb, limb_bits))
    ok = True
    for c, v in zip(trace.cts, res):
        put("results", *P.expand_assign_cells(v, L, limb_bits, lb))
        ae, bit = P.expand_assert_equal_fresh_cells(P.decompose_biguint(c, L, limb_bits), P.decompose_biguint(v, L, limb_bits))
        put("results", ae)
        ok = ok and bool(bit)
    seg["end"] = (len(adv), len(lk))
    seg["satisfied"] = ok
    return [v % R for v in adv], [v % R for v in lk], seg


def sballot_gate_mask(count: int, m_bits: int, s_limbs: int, enc_bits: int, limb_bits: int, lb: int) -> np.ndarray:
    """uint8 selector over the advice stream (1 where a gate window starts), from the gate_offsets_* functions"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln

    def mask(part):
        g, n = part
        m = np.zeros(n, dtype=np.uint8)
        m[np.asarray(g, dtype=np.int64)] = 1
        return m

    narrow = mask(P.gate_offsets_assign(Ln, limb_bits, lb))
    wide = mask(P.gate_offsets_assign(L, limb_bits, lb))
    s_asg = mask(P.gate_offsets_assign(s_limbs, limb_bits, lb))
    mm = mask(P.gate_offsets_mul_mod(L, lb, limb_bits))
    parts = [narrow, narrow, wide, np.zeros(count, dtype=np.uint8)]     # n, g, hs; load_witness: no gate
    if count >= 2:
        parts.append(mask(([3 * i for i in range(count - 1)], 1 + 3 * (count - 1))))
    parts += [s_asg] * count
    parts.append(mask(P.gate_offsets_square(Ln)))
    parts.append(mask(P.gate_offsets_refresh(P.refresh_aux(limb_bits, Ln, Ln), limb_bits, lb)))
    parts.append(np.zeros(1, dtype=np.uint8))                            # load_zero
    two = np.zeros(2, dtype=np.uint8)
    ntb = lambda W: mask(([3 * i for i in range(W - 1)] + [1 + 3 * (W - 1) + 4 * i for i in range(W)], 7 * W - 2))
    sel = mask(([8 * t + o for t in range(L) for o in (0, 4)], 8 * L))
    limb = np.concatenate([ntb(limb_bits)] + [mm, sel, mm] * limb_bits)
    entry = np.concatenate([two, ntb(m_bits)] + [mm, sel, mm] * m_bits + [two] + [limb] * s_limbs + [mm])
    parts += [entry] * count
    parts += [wide, mask(P.gate_offsets_assert_equal(L))] * count
    return np.concatenate(parts)


def statement(n: int, g: int, hs: int, cts: Sequence[int], total, enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | g[Ln] | hs[2 Ln] | c_1[2 Ln] | .. | c_K[2 Ln] | S (K >= 2 only: total is None for K = 1), little-endian limbs"""
    Ln = enc_bits // limb_bits
    out = P.decompose_biguint(n, Ln, limb_bits) + P.decompose_biguint(g, Ln, limb_bits) + P.decompose_biguint(hs, 2 * Ln, limb_bits)
    for v in cts:
        out += P.decompose_biguint(v, 2 * Ln, limb_bits)
    assert (total is None) == (len(cts) == 1)
    if total is not None:
        out.append(int(total))
    return out
