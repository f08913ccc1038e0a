"""Test-side restatement of the packed ballot (circuit kind 11 / "pballot"), independent of the product: the
scheme in Python integers (M = sum_j v_j 2^(j w), c = g^M hs^s mod n^2 = (prod_j G_j^v_j) hs^s with G_j = g^(2^(j w))), the trace of R
ciphertexts of K slots under one key -- per slot oracle.pyref.pow_mod_uniform_trace over b bits of v_ij on the base G_j, the same over
s_bits bits of s_i on the base hs, and K mul_mod_steps that fold the K + 1 powers --, and the cell stream composed from oracle.pyref's
per-operation emitters with its gate mask from the gate_offsets_* functions.  Python integers throughout.  The product must not import
this module.

Record order: ciphertext-major, 2 b K + 2 s_bits + K per entry: the K slot chains' 2 b records each (bit t: (acc, sq, q, r) then
(sq, sq, q, sq')), the hs-chain's 2 s_bits in the same form, then the folds (P_0, P_1), (t_1, P_2), .., (t_{K-1}, hss); K = 1: (P_0, hss)."""
from typing import List, NamedTuple, Sequence

import numpy as np

from oracle import pyref as P
from tests.sballot_ref import SAFE_P, SAFE_Q, decrypt, djn_h, djn_hs  # noqa: F401  (the key material and the scheme's decryption)
from tests.tally_ref import check_columns, place  # noqa: F401  (re-exported: the tests take them from here)

R = P.FR_R


# ------------------------------------------------------------------------------------------------ the scheme
def pack(values: Sequence[int], w: int) -> int:
    assert all(0 <= v < (1 << w) for v in values)
    return sum(v << (j * w) for j, v in enumerate(values))


def unpack(M: int, K: int, w: int) -> List[int]:
    return [(M >> (j * w)) & ((1 << w) - 1) for j in range(K)]


def bases(n: int, g: int, K: int, w: int) -> List[int]:
    return [pow(g, 1 << (j * w), n * n) for j in range(K)]


def encrypt(n: int, g: int, hs: int, values: Sequence[int], w: int, s: int) -> int:
    return pow(g, pack(values, w), n * n) * pow(hs, s, n * n) % (n * n)


def capacity(w: int, b: int) -> int:
    return ((1 << w) - 1) // ((1 << b) - 1)


# ------------------------------------------------------------------------------------------------ the trace
class Trace(NamedTuple):
    cts: List[int]                        # what each entry's last fold leaves
    v_chains: List[List[List[P.Step]]]    # [R][K]: 2 b steps each
    s_chains: List[List[P.Step]]          # [R]: 2 s_bits steps each
    folds: List[List[P.Step]]             # [R][K]
    v_exps: List[List[int]]               # what each slot chain was run with
    s_exps: List[int]                     # what each hs-chain was run with
    totals: List[int]                     # the last cell of each sum (K = 1: unused)


def per_entry(K: int, m_bits: int, s_bits: int) -> int:
    return 2 * m_bits * K + 2 * s_bits + K


def pballot_trace(n: int, hs: int, gs: Sequence[int], vs: Sequence[Sequence[int]], ss: Sequence[int], m_bits: int, s_bits: int,
                  forge=None) -> Trace:
    """forge, everything downstream of it recomputed consistently (the soundness negatives):
      ('val', i, j, v')      slot chain (i, j) runs with v' while the load_witness cell keeps v_ij
      ('base', i, j, delta)  slot chain (i, j)'s first sq is G_j + delta
      ('swap', i)            slot 0's chain of ciphertext i runs on G_1 (the base swap)
      ('fold', i, q, delta)  fold q's second operand is the power it names + delta
      ('s', i, s')           hs-chain i runs with s' while assign_integer(s_i) keeps s_i
      ('sum', i, delta)      the last cell of ciphertext i's sum is S_i + delta"""
    n2 = n * n
    K = len(gs)
    assert len(vs) == len(ss) >= 1 and all(len(row) == K for row in vs)
    t = Trace([], [], [], [], [], [], [])
    for i, (row, s) in enumerate(zip(vs, ss)):
        hit = lambda name: forge is not None and forge[0] == name and forge[1] == i
        powers, chains, exps = [], [], []
        for j, v in enumerate(row):
            ve = forge[3] if hit("val") and forge[2] == j else v
            base = gs[j] + (forge[3] if hit("base") and forge[2] == j else 0)
            if hit("swap") and j == 0:
                base = gs[1]
            pj, sv = P.pow_mod_uniform_trace(base, ve, m_bits, n2)
            assert len(sv) == 2 * m_bits
            powers.append(pj)
            chains.append(sv)
            exps.append(ve)
        se = forge[2] if hit("s") else s
        hss, sh = P.pow_mod_uniform_trace(hs, se, s_bits, n2)
        assert len(sh) == 2 * s_bits
        run, folds = powers[0], []
        for q in range(K):
            other = (powers[q + 1] if q + 1 < K else hss) + (forge[3] if hit("fold") and forge[2] == q else 0)
            st = P.mul_mod_step(run, other, n2)
            folds.append(st)
            run = st[3]
        t.cts.append(run)
        t.v_chains.append(chains)
        t.s_chains.append(sh)
        t.folds.append(folds)
        t.v_exps.append(exps)
        t.s_exps.append(se)
        t.totals.append(sum(row) + (forge[2] if hit("sum") else 0))
    return t


def records(trace: Trace) -> List[P.Step]:
    """the records in pz_paillier_pballot's order"""
    out: List[P.Step] = []
    for chains, sh, folds in zip(trace.v_chains, trace.s_chains, trace.folds):
        for sv in chains:
            out += list(sv)
        out += list(sh) + list(folds)
    return out


# ------------------------------------------------------------------------------------------------ the circuit
def pballot_cells(n: int, hs: int, gs: Sequence[int], vs: Sequence[Sequence[int]], ss: Sequence[int], res: Sequence[int], m_bits: int,
                  s_limbs: int, enc_bits: int, limb_bits: int, lb: int, trace: Trace = None):
    """the stream: assign n; assign hs and G_0 .. G_{K-1} at full width; load_witness of the R K values, ciphertext-major; for K >= 2 one
    FlexGate::sum per ciphertext; assign s_1 .. s_R (s_limbs limbs each); square + refresh once, load_zero; per ciphertext, per slot
    [1, 0], num_to_bits(v, b) and b blocks, then [1, 0] and pow_mod(hs, s_i) limb by limb, then the K fold blocks; per ciphertext assign
    res_i and assert_equal_fresh(c_i, res_i).
    trace = pballot_trace's result to expand (default: the honest one).  The load_witness cells, the sums' operands and the
    assign_integer(s_i) always hold `vs` and `ss`; a chain's num_to_bits holds the exponent its records were run with.
    -> (advice cells, lookup cells, {name: (advice offset, lookup offset)}) as canonical integers"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    n2 = n * n
    Rn, K = len(vs), len(gs)
    s_bits = s_limbs * limb_bits
    if trace is None:
        trace = pballot_trace(n, hs, gs, vs, ss, m_bits, s_bits)
    assert len(trace.cts) == len(ss) == len(res) == Rn
    adv: List[int] = []
    lk: List[int] = []
    seg = {}

    def put(name, a, l=()):
        seg.setdefault(name, (len(adv), len(lk)))
        adv.extend(a)
        lk.extend(l)

    put("assign_n", *P.expand_assign_cells(n, Ln, limb_bits, lb))
    put("assign_hs", *P.expand_assign_cells(hs, L, limb_bits, lb))
    for gj in gs:
        put("assign_bases", *P.expand_assign_cells(gj, L, limb_bits, lb))
    put("values", [int(v) for row in vs for v in row])
    if K >= 2:
        for row, total in zip(vs, trace.totals):
            cells, s = [int(row[0])], int(row[0])
            for j in range(1, K):
                s += int(row[j])
                cells += [1, int(row[j]), s]
            cells[-1] = total
            assert len(cells) == 1 + 3 * (K - 1)
            put("sums", cells)
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

    for chains, sh, folds, ves, se in zip(trace.v_chains, trace.s_chains, trace.folds, trace.v_exps, trace.s_exps):
        for sv, ve in zip(chains, ves):
            put("entries", [1, 0])
            nb_cells, bits = P._num_to_bits_cells(ve, m_bits)
            assert len(nb_cells) == 7 * m_bits - 2
            put("entries", nb_cells)
            bit_blocks(sv, bits, 0)
        put("entries", [1, 0])
        sl = P.decompose_biguint(se, s_limbs, limb_bits)
        for li in range(s_limbs):
            nb_cells, bits = P._num_to_bits_cells(sl[li], limb_bits)
            put("entries", nb_cells)
            bit_blocks(sh, bits, li * limb_bits)
        for st in folds:
            put("entries", *P.expand_mul_mod_cells(*st, n2, L, lb, limb_bits))
    ok = True
    for c, v in zip(trace.cts, res):
        put("results", *P.expand_assign_cells(v, L, limb_bits, lb))
        ae, bit = P.expand_assert_equal_fresh_cells(P.decompose_biguint(c, L, limb_bits), P.decompose_biguint(v, L, limb_bits))
        put("results", ae)
        ok = ok and bool(bit)
    seg["end"] = (len(adv), len(lk))
    seg["satisfied"] = ok
    return [v % R for v in adv], [v % R for v in lk], seg


def pballot_gate_mask(count: int, slots: int, m_bits: int, s_limbs: int, enc_bits: int, limb_bits: int, lb: int) -> np.ndarray:
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
    parts = [narrow] + [wide] * (1 + slots) + [np.zeros(count * slots, dtype=np.uint8)]     # n; hs, G_j; load_witness: no gate
    if slots >= 2:
        parts += [mask(([3 * i for i in range(slots - 1)], 1 + 3 * (slots - 1)))] * count
    parts += [s_asg] * count
    parts.append(mask(P.gate_offsets_square(Ln)))
    parts.append(mask(P.gate_offsets_refresh(P.refresh_aux(limb_bits, Ln, Ln), limb_bits, lb)))
    parts.append(np.zeros(1, dtype=np.uint8))                            # load_zero
    two = np.zeros(2, dtype=np.uint8)
    ntb = lambda W: mask(([3 * i for i in range(W - 1)] + [1 + 3 * (W - 1) + 4 * i for i in range(W)], 7 * W - 2))
    sel = mask(([8 * t + o for t in range(L) for o in (0, 4)], 8 * L))
    limb = np.concatenate([ntb(limb_bits)] + [mm, sel, mm] * limb_bits)
    slot = np.concatenate([two, ntb(m_bits)] + [mm, sel, mm] * m_bits)
    entry = np.concatenate([slot] * slots + [two] + [limb] * s_limbs + [mm] * slots)
    parts += [entry] * count
    parts += [wide, mask(P.gate_offsets_assert_equal(L))] * count
    return np.concatenate(parts)


def statement(n: int, hs: int, gs: Sequence[int], cts: Sequence[int], totals, enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | hs[2 Ln] | G_0[2 Ln] | .. | G_{K-1}[2 Ln] | c_1[2 Ln] | .. | c_R[2 Ln] | S_1 | .. | S_R (K >= 2 only: totals is None for
    K = 1), little-endian limbs"""
    Ln = enc_bits // limb_bits
    out = P.decompose_biguint(n, Ln, limb_bits) + P.decompose_biguint(hs, 2 * Ln, limb_bits)
    for v in list(gs) + list(cts):
        out += P.decompose_biguint(v, 2 * Ln, limb_bits)
    assert (totals is None) == (len(gs) == 1)
    if totals is not None:
        assert len(totals) == len(cts)
        out += [int(t) for t in totals]
    return out
