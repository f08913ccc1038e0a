"""Test-side restatement of the short-randomness mix (circuit kind 10 / "smix"), independent of the product:
K = 2^d ciphertexts under one key (n, hs) go through the Benes network of tests/mix_ref.py and leave as c'_i = d_i hs^s_i mod n^2, d_i
the network's output at position i, s_i < 2^s_bits.  The network (rules, routing, switch cells) is mix_ref's; a chain is
oracle.pyref.pow_mod_uniform_trace over s_bits bits of s_i on the base hs, as tests/sballot_ref.py runs its hs-chain; then one
mul_mod_step.  The cell stream is composed from oracle.pyref's per-operation emitters, its gate mask from the gate_offsets_*
functions.  Python integers throughout.  The product must not import this module.

Record order: output-major, 2 s_bits + 1 per output: the chain's 2 s_bits records (bit j: (acc, sq, q, r) then (sq, sq, q, sq')), then
(d_i, hss_i, q, c'_i)."""
from typing import List, NamedTuple, Sequence

import numpy as np

from oracle import circuit as CQ
from oracle import pyref as P
from tests import mix_ref as MR
from tests.mix_ref import Switch, apply, benes_layers, n_bits, route  # noqa: F401  (re-exported: the network is the mix's)
from tests.sballot_ref import SAFE_P, SAFE_Q, decrypt, djn_h, djn_hs, encrypt  # noqa: F401  (re-exported: the scheme is the ballot's)
from tests.tally_ref import check_columns, place  # noqa: F401  (re-exported: the tests take them from here)

R = P.FR_R

NETWORK_FORGES = ("bit", "dup", "src", "in")


class Trace(NamedTuple):
    layers: List[List[int]]        # every layer's values ([] for K = 1)
    routed: List[int]              # d_i: what the final block of output i multiplies
    s_chains: List[List[P.Step]]   # 2 s_bits steps each
    finals: List[P.Step]
    mixed: List[int]               # c'_i
    switches: List[List[Switch]]   # per layer, in switch order, limb by limb
    last: List[List[int]]          # the limbs the last layer leaves at every position (K = 1: c_1's)
    s_exps: List[int]              # what each chain was run with


def per_output(s_bits: int) -> int:
    return 2 * s_bits + 1


def smix_trace(n: int, hs: int, cts: Sequence[int], bits: Sequence[int], ss: Sequence[int], s_bits: int, forge=None, limb_bits: int = 64,
               limbs: int = 0) -> Trace:
    """forge, everything downstream of it recomputed consistently (the soundness negatives):
      ('bit', l, s, 2)    switch s of layer l holds the bit 2
      ('dup', l, s)       the switch's two selects run under different bits: one input leaves twice, the other is dropped
      ('src', l, j, 1)    the selects of layer l read, for position j, the previous layer's limb 0 plus 1
      ('in', j, 1)        layer 0 reads c_j + 1 while the assigned (exposed) cells keep c_j
      ('s', i, s')        chain i runs with s' while assign_integer(s_i) keeps s_i
      ('base', i, delta)  chain i's first sq is hs + delta
      ('hss', i, delta)   the final block's second operand is hss_i + delta
      ('d', i, delta)     the final block's first operand is d_i + delta"""
    n2 = n * n
    K = len(cts)
    assert K == len(ss) >= 1
    net = MR.mix_trace(n, cts, bits, [1] * K, forge=forge if forge is not None and forge[0] in NETWORK_FORGES else None,
                       limb_bits=limb_bits, limbs=limbs)
    t = Trace(net.layers, net.routed, [], [], [], net.switches, net.last, [])
    for i, (d, s) in enumerate(zip(net.routed, ss)):
        hit = lambda name: forge is not None and forge[0] == name and forge[1] == i
        se = forge[2] if hit("s") else s
        hss, sh = P.pow_mod_uniform_trace(hs + (forge[2] if hit("base") else 0), se, s_bits, n2)
        assert len(sh) == 2 * s_bits
        fin = P.mul_mod_step(d + (forge[2] if hit("d") else 0), hss + (forge[2] if hit("hss") else 0), n2)
        t.s_chains.append(sh)
        t.finals.append(fin)
        t.mixed.append(fin[3])
        t.s_exps.append(se)
    return t


def records(trace: Trace) -> List[P.Step]:
    """the records in pz_paillier_smix's order"""
    out: List[P.Step] = []
    for sh, fin in zip(trace.s_chains, trace.finals):
        out += list(sh) + [fin]
    return out


def smix_cells(n: int, hs: int, cts: Sequence[int], ss: Sequence[int], res: Sequence[int], s_limbs: int, enc_bits: int, limb_bits: int,
               lb: int, trace: Trace):
    """the stream of `trace` (smix_trace(.., s_limbs * limb_bits, limb_bits=limb_bits, limbs=2 * enc_bits // limb_bits)): assign n;
    assign hs, c_1 .. c_K at full width; assign s_1 .. s_K (s_limbs limbs each); square + refresh once, load_zero; the network; per
    output [1, 0], per limb of s_i num_to_bits and that limb's blocks, mul_mod(d_i, hss_i); per output assign c'_i and
    assert_equal_fresh.  The assigned cells always hold `hs`, `cts`, `ss` and `res`; a switch's cells hold what the trace's selects
    read and left, a chain's num_to_bits the exponent its records were run with.
    -> (advice cells, lookup cells, {name: (advice offset, lookup offset)}) as canonical integers"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    n2 = n * n
    K = len(cts)
    assert len(ss) == len(res) == len(trace.mixed) == K and all(len(ls) == L for ls in trace.last)
    adv: List[int] = []
    lk: List[int] = []
    seg = {}

    def put(name, a, l=()):
        seg.setdefault(name, (len(adv), len(lk)))
        adv.extend(a)
        lk.extend(l)

    put("assign_n", *P.expand_assign_cells(n, Ln, limb_bits, lb))
    put("assign_hs", *P.expand_assign_cells(hs, L, limb_bits, lb))
    for c in cts:
        put("assign_cts", *P.expand_assign_cells(c, L, limb_bits, lb))
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
    seg["network"] = (len(adv), len(lk))
    for row in trace.switches:
        for sw in row:
            put("network", [0, sw.bit, sw.bit, sw.bit])
            for t in range(L):
                put("network", P._select_cells(sw.in_jp[t], sw.in_j[t], sw.sel[0]))
                put("network", P._select_cells(sw.in_j[t], sw.in_jp[t], sw.sel[1]))
    seg["outputs"] = (len(adv), len(lk))
    for sh, fin, se in zip(trace.s_chains, trace.finals, trace.s_exps):
        put("outputs", [1, 0])
        sl = P.decompose_biguint(se, s_limbs, limb_bits)
        for li in range(s_limbs):
            nb_cells, bits = P._num_to_bits_cells(sl[li], limb_bits)
            assert len(nb_cells) == 7 * limb_bits - 2
            put("outputs", nb_cells)
            for j, bit in enumerate(bits):
                st_mul, st_sq = sh[2 * (li * limb_bits + j)], sh[2 * (li * limb_bits + j) + 1]
                put("outputs", *P.expand_mul_mod_cells(*st_mul, n2, L, lb, limb_bits))
                acc_l, mul_l = P.decompose_biguint(st_mul[0], L, limb_bits), P.decompose_biguint(st_mul[3], L, limb_bits)
                for t in range(L):
                    put("outputs", P._select_cells(mul_l[t], acc_l[t], bit))
                put("outputs", *P.expand_mul_mod_cells(*st_sq, n2, L, lb, limb_bits))
        put("outputs", *P.expand_mul_mod_cells(*fin, n2, L, lb, limb_bits))
    ok = True
    for c, v in zip(trace.mixed, res):
        put("results", *P.expand_assign_cells(v, L, limb_bits, lb))
        ae, bit = P.expand_assert_equal_fresh_cells(P.decompose_biguint(c, L, limb_bits), P.decompose_biguint(v, L, limb_bits))
        put("results", ae)
        ok = ok and bool(bit)
    seg["end"] = (len(adv), len(lk))
    seg["satisfied"] = ok
    return [v % R for v in adv], [v % R for v in lk], seg


def smix_gate_mask(count: int, s_limbs: int, enc_bits: int, limb_bits: int, lb: int) -> np.ndarray:
    """the structure: uint8 selector over the advice stream (1 where a gate window starts), from the gate_offsets_* functions"""
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
    parts = [narrow] + [wide] * (1 + count) + [s_asg] * count
    parts.append(mask(P.gate_offsets_square(Ln)))
    parts.append(mask(P.gate_offsets_refresh(P.refresh_aux(limb_bits, Ln, Ln), limb_bits, lb)))
    parts.append(np.zeros(1, dtype=np.uint8))                            # load_zero
    switch = mask(([0] + [4 + 8 * t + o for t in range(2 * L) for o in (0, 4)], 4 + 16 * L))
    parts += [switch] * n_bits(count)
    two = np.zeros(2, dtype=np.uint8)
    W = limb_bits
    ntb = mask(([3 * i for i in range(W - 1)] + [1 + 3 * (W - 1) + 4 * i for i in range(W)], 7 * W - 2))
    sel = mask(([8 * t + o for t in range(L) for o in (0, 4)], 8 * L))
    limb = np.concatenate([ntb] + [mm, sel, mm] * W)
    parts += [np.concatenate([two] + [limb] * s_limbs + [mm])] * count
    parts += [wide, mask(P.gate_offsets_assert_equal(L))] * count
    return np.concatenate(parts)


def public_cells(count: int, s_limbs: int, enc_bits: int, limb_bits: int, lb: int) -> List[int]:
    """the stream indices of the statement's cells: the limb cells that head the assign_integer of n, hs, every c_j and every c'_i"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    narrow = P.gate_offsets_assign(Ln, limb_bits, lb)[1]
    wide = P.gate_offsets_assign(L, limb_bits, lb)[1]
    eq = P.gate_offsets_assert_equal(L)[1]
    total = smix_gate_mask(count, s_limbs, enc_bits, limb_bits, lb).shape[0]
    res0 = total - count * (wide + eq)
    out = list(range(Ln))
    for i in range(1 + count):
        out += [narrow + i * wide + j for j in range(L)]
    for i in range(count):
        out += [res0 + i * (wide + eq) + j for j in range(L)]
    return out


def mock_prover(selectors, map_col, map_row, cols, n_lk: int, k: int, lb: int, blinding_factors: int = 6) -> List[str]:
    """oracle.circuit.mock_prover (the MockProver analogue: every enabled gate, every equality constraint, every lookup cell in the
    table) on placed columns under a structure given as selectors and a permutation: the equalities are the permutation's moved cells
    against their images.  -> the failures, each beginning 'gate', 'copy' or 'lookup' (empty = satisfied)"""
    sel = np.asarray(selectors)
    mc, mr = np.asarray(map_col).astype(np.int64), np.asarray(map_row).astype(np.int64)
    N = 1 << k
    eqs = []
    for j in range(mc.shape[0]):
        for r in np.nonzero((mc[j] != j) | (mr[j] != np.arange(N)))[0].tolist():
            eqs.append(((j, r), (int(mc[j, r]), int(mr[j, r]))))
    st = CQ.Structure(k=k, lookup_bits=lb, max_rows=N - (blinding_factors + 3), blinding_factors=blinding_factors, starts=[], n_adv=sel.shape[0],
                      n_lk=n_lk, selectors=sel, constants=[], table=[i if i < (1 << lb) else 0 for i in range(N)], map_col=mc, map_row=mr,
                      equalities=eqs, adv_cols=[], lk_cols=[])
    return CQ.mock_prover(st, [list(c) for c in cols])


def statement(n: int, hs: int, cts: Sequence[int], mixed: Sequence[int], enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | hs[2 Ln] | c_1[2 Ln] | .. | c_K[2 Ln] | c'_1[2 Ln] | .. | c'_K[2 Ln], little-endian limbs"""
    Ln = enc_bits // limb_bits
    out = P.decompose_biguint(n, Ln, limb_bits)
    for v in [hs] + list(cts) + list(mixed):
        out += P.decompose_biguint(v, 2 * Ln, limb_bits)
    return out
