"""Test-side restatement of the ballot circuit (kind 6 / "ballot"), independent of the product: K ciphertexts
c_i = g^m_i r_i^n mod n^2 under one key, every m_i below 2^b, and for K >= 2 the public sum S of the m_i.  Per ciphertext
oracle.pyref.pow_mod_uniform_trace over b message bits, pow_mod_fixed_exp_trace over n's bits and one mul_mod_step; the cell stream is
composed from oracle.pyref's per-operation emitters and its gate mask from the gate_offsets_* functions.  Python integers throughout.
The product must not import this module.

Record order: ciphertext-major, 2 b + nr + 1 per entry (nr = bits(n) + popcount(n)): the g-chain's 2 b records (bit j: (acc, sq, q, r)
then (sq, sq, q, sq')), the r-chain's nr in pow_mod_fixed_exp_trace order, the final (gm, rn, q, c)."""
from typing import List, NamedTuple, Sequence

import numpy as np

from oracle import pyref as P
from tests.tally_ref import check_columns, place  # noqa: F401  (re-exported: the tests take them from here)

R = P.FR_R


class Trace(NamedTuple):
    cts: List[int]                 # what each entry's final block leaves
    g_chains: List[List[P.Step]]   # 2 b steps each
    r_chains: List[List[P.Step]]   # nr steps each
    finals: List[P.Step]
    exponents: List[int]           # what each g-chain was run with
    bases: List[int]               # each g-chain's first sq
    total: int                     # the last cell of the sum (K = 1: unused, the message)


def n_steps_r(n: int) -> int:
    return n.bit_length() + bin(n).count("1")


def ballot_trace(n: int, g: int, ms: Sequence[int], rs: Sequence[int], m_bits: int, forge=None) -> Trace:
    """forge, everything downstream of it recomputed consistently (the soundness negatives):
      ('exp', i, m')     chain i runs with m' while the load_witness cell keeps m_i
      ('base', i, delta) chain i's first sq is g + delta
      ('rn', i, delta)   the final block's second operand is rn_i + delta
      ('sum', delta)     the last sum cell is S + delta"""
    n2 = n * n
    assert len(ms) == len(rs) >= 1
    t = Trace([], [], [], [], [], [], sum(ms) + (forge[1] if forge is not None and forge[0] == "sum" else 0))
    for i, (m, r) in enumerate(zip(ms, rs)):
        hit = forge is not None and forge[0] != "sum" and forge[1] == i
        e = forge[2] if hit and forge[0] == "exp" else m
        base = g + forge[2] if hit and forge[0] == "base" else g
        gm, sg = P.pow_mod_uniform_trace(base, e, m_bits, n2)
        rn, sr = P.pow_mod_fixed_exp_trace(r, n, n2)
        assert len(sg) == 2 * m_bits and len(sr) == n_steps_r(n)
        fin = P.mul_mod_step(gm, rn + forge[2] if hit and forge[0] == "rn" else rn, n2)
        t.cts.append(fin[3])
        t.g_chains.append(sg)
        t.r_chains.append(sr)
        t.finals.append(fin)
        t.exponents.append(e)
        t.bases.append(base)
    return t


def records(trace: Trace) -> List[P.Step]:
    """the records in pz_paillier_ballot's order"""
    out: List[P.Step] = []
    for sg, sr, fin in zip(trace.g_chains, trace.r_chains, trace.finals):
        out += list(sg) + list(sr) + [fin]
    return out


def ballot_cells(n: int, g: int, ms: Sequence[int], rs: Sequence[int], res: Sequence[int], m_bits: int, enc_bits: int, limb_bits: int,
                 lb: int, trace: Trace = None):
    """the stream: assign n, g; load_witness(m_1 .. m_K); for K >= 2 FlexGate::sum of them; assign r_1 .. r_K; square + refresh once,
    load_zero; per ciphertext pow_mod(g_ext, m_i) over b bits, pow_mod_fixed_exp(r_i_ext, n), mul_mod; per ciphertext assign res_i and
    assert_equal_fresh(c_i, res_i).
    trace = ballot_trace's result to expand (default: the honest one).  The load_witness cells and the sum's operands always hold `ms`; a
    chain's num_to_bits holds the exponent its records were run with.
    -> (advice cells, lookup cells, {name: (advice offset, lookup offset)}) as canonical integers"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    n2 = n * n
    K = len(ms)
    if trace is None:
        trace = ballot_trace(n, g, ms, rs, m_bits)
    assert len(trace.cts) == len(rs) == len(res) == K
    adv: List[int] = []
    lk: List[int] = []
    seg = {}

    def put(name, a, l=()):
        seg.setdefault(name, (len(adv), len(lk)))
        adv.extend(a)
        lk.extend(l)

    put("assign_n", *P.expand_assign_cells(n, Ln, limb_bits, lb))
    put("assign_g", *P.expand_assign_cells(g, Ln, limb_bits, lb))
    put("messages", [int(m) for m in ms])
    if K >= 2:
        cells, s = [int(ms[0])], int(ms[0])
        for i in range(1, K):
            s += int(ms[i])
            cells += [1, int(ms[i]), s]
        cells[-1] = trace.total
        assert len(cells) == 1 + 3 * (K - 1)
        put("sum", cells)
    for r in rs:
        put("assign_rs", *P.expand_assign_cells(r, Ln, limb_bits, lb))
    nl = P.decompose_biguint(n, Ln, limb_bits)
    sq_cells, prod = P._mul_cells(nl, nl, 2 * Ln - 1)
    put("square", sq_cells)
    inc = P.refresh_aux(limb_bits, Ln, Ln)
    assert len(inc) == L
    r_adv, r_lk, fresh = P.expand_refresh_cells(prod, inc, limb_bits, lb)
    assert P.get_biguint(fresh, limb_bits) == n2
    put("refresh", r_adv, r_lk)
    put("load_zero", [0])
    for sg, sr, fin, e in zip(trace.g_chains, trace.r_chains, trace.finals, trace.exponents):
        put("entries", [1, 0])
        nb_cells, bits = P._num_to_bits_cells(e, m_bits)
        assert len(nb_cells) == 7 * m_bits - 2
        put("entries", nb_cells)
        for j in range(m_bits):
            st_mul, st_sq = sg[2 * j], sg[2 * j + 1]
            put("entries", *P.expand_mul_mod_cells(*st_mul, n2, L, lb, limb_bits))
            acc_l, mul_l = P.decompose_biguint(st_mul[0], L, limb_bits), P.decompose_biguint(st_mul[3], L, limb_bits)
            for t in range(L):
                put("entries", P._select_cells(mul_l[t], acc_l[t], bits[j]))
            put("entries", *P.expand_mul_mod_cells(*st_sq, n2, L, lb, limb_bits))
        put("entries", [1, 0])
        for st in sr:
            put("entries", *P.expand_mul_mod_cells(*st, n2, L, lb, limb_bits))
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


def ballot_gate_mask(count: int, m_bits: int, enc_bits: int, limb_bits: int, lb: int, n_steps_r_: int) -> np.ndarray:
    """uint8 selector over the advice stream (1 where a gate window starts), from the gate_offsets_* functions"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    W = m_bits

    def mask(part):
        g, n = part
        m = np.zeros(n, dtype=np.uint8)
        m[np.asarray(g, dtype=np.int64)] = 1
        return m

    narrow = mask(P.gate_offsets_assign(Ln, limb_bits, lb))
    wide = mask(P.gate_offsets_assign(L, limb_bits, lb))
    mm = mask(P.gate_offsets_mul_mod(L, lb, limb_bits))
    parts = [narrow, narrow, np.zeros(count, dtype=np.uint8)]            # n, g; load_witness: no gate
    if count >= 2:
        parts.append(mask(([3 * i for i in range(count - 1)], 1 + 3 * (count - 1))))
    parts += [narrow] * count
    parts.append(mask(P.gate_offsets_square(Ln)))
    parts.append(mask(P.gate_offsets_refresh(P.refresh_aux(limb_bits, Ln, Ln), limb_bits, lb)))
    parts.append(np.zeros(1, dtype=np.uint8))                            # load_zero
    two = np.zeros(2, dtype=np.uint8)
    ntb = mask(([3 * i for i in range(W - 1)] + [1 + 3 * (W - 1) + 4 * i for i in range(W)], 7 * W - 2))
    sel = mask(([8 * t + o for t in range(L) for o in (0, 4)], 8 * L))
    entry = np.concatenate([two, ntb] + [mm, sel, mm] * W + [two] + [mm] * (n_steps_r_ + 1))
    parts += [entry] * count
    parts += [wide, mask(P.gate_offsets_assert_equal(L))] * count
    return np.concatenate(parts)


def statement(n: int, g: int, cts: Sequence[int], total, enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | g[Ln] | c_1[2 Ln] | .. | c_K[2 Ln] | S (K >= 2 only: total is None for K = 1), little-endian limbs"""
    Ln = enc_bits // limb_bits
    out = P.decompose_biguint(n, Ln, limb_bits) + P.decompose_biguint(g, Ln, limb_bits)
    for v in cts:
        out += P.decompose_biguint(v, 2 * Ln, limb_bits)
    assert (total is None) == (len(cts) == 1)
    if total is not None:
        out.append(int(total))
    return out
