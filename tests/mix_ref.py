"""Test-side restatement of the mix, independent of the product: K = 2^d ciphertexts under one key go through
a Benes network of conditional swaps and leave as c'_i = d_i r_i^n mod n^2, d_i the network's output at position i.  The network is
written down from its rules (benes_layers), applied in Python integers (apply) and routed by a recursive looping algorithm of this
module's own (route: a two-colouring of the constraint graph, then the two inner networks).  Per output
oracle.pyref.pow_mod_fixed_exp_trace over n's bits and one mul_mod_step.  The product must not import this module.

The rules: d = log2 K, 2d - 1 layers; layer l acts on bit beta(l) = l for l < d and 2d - 2 - l above; switch s of a layer is the s-th
position j, ascending, with bit beta clear, its partner j' = j | 2^beta; with bit b: out[j] = b ? in[j'] : in[j], out[j'] = b ? in[j] :
in[j'].  Values stay in place.  Bits layer-major, (2d - 1) K / 2 in all.  perm[i] = the index of the input that output i receives.

The cell stream (mix_cells) is composed from oracle.pyref's per-operation emitters, its gate mask (mix_gate_mask) from the
gate_offsets_* functions: assign n; assign c_1 .. c_K at full width; assign r_1 .. r_K; square + refresh of n, once; load_zero; per
switch [0, b, b, b] and per limb select(in[j'], in[j], b) then select(in[j], in[j'], b); per output [1, 0], the r^n chain's blocks
and mul_mod(d_i, rn_i); per output assign c'_i at full width and assert_equal_fresh.

Record order: output-major, nr + 1 per output (nr = bits(n) + popcount(n)): the r-chain's nr in pow_mod_fixed_exp_trace order, then
(d_i, rn_i, q, c'_i)."""
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from oracle import pyref as P
from tests.tally_ref import check_columns, place  # noqa: F401  (re-exported: the tests take them from here)

R = P.FR_R


def n_steps_r(n: int) -> int:
    return n.bit_length() + bin(n).count("1")


def benes_layers(K: int) -> List[List[Tuple[int, int]]]:
    """per layer the switches (j, j') in switch order"""
    assert K >= 1 and K & (K - 1) == 0
    d = K.bit_length() - 1
    out = []
    for l in range(2 * d - 1):
        beta = l if l < d else 2 * d - 2 - l
        out.append([(j, j | (1 << beta)) for j in range(K) if not (j >> beta) & 1])
    return out


def n_bits(K: int) -> int:
    return sum(len(layer) for layer in benes_layers(K))


def apply(bits: Sequence[int], xs: Sequence) -> List[list]:
    """every layer's outputs ([] for K = 1); the network's result is the last one"""
    layers, cur, at = [], list(xs), 0
    for layer in benes_layers(len(xs)):
        nxt = list(cur)
        for j, jp in layer:
            if bits[at]:
                nxt[j], nxt[jp] = cur[jp], cur[j]
            at += 1
        layers.append(nxt)
        cur = nxt
    assert at == len(bits)
    return layers


def _route(perm: List[int]) -> List[List[int]]:
    """the layers' bits of the network over len(perm) positions, recursively: outer layers pair neighbours, the inner networks live on
    the even (colour 0) and the odd (colour 1) positions, whose switch s is the parent's switch 2 s + colour"""
    K = len(perm)
    if K == 1:
        return []
    if K == 2:
        return [[int(perm[0] == 1)]]
    # two-colour the inputs: the inputs of one input switch differ, and so do the inputs bound for one output switch
    nbr = [[] for _ in range(K)]
    for k in range(K // 2):
        for a, b in ((2 * k, 2 * k + 1), (perm[2 * k], perm[2 * k + 1])):
            nbr[a].append(b)
            nbr[b].append(a)
    colour = [None] * K
    for start in range(K):
        if colour[start] is not None:
            continue
        colour[start] = 0
        stack = [start]
        while stack:
            a = stack.pop()
            for b in nbr[a]:
                if colour[b] is None:
                    colour[b] = 1 - colour[a]
                    stack.append(b)
                else:
                    assert colour[b] != colour[a]
    first = [colour[2 * k] for k in range(K // 2)]                   # input 2k leaves for the odd network: the switch crosses
    last = [colour[perm[2 * k]] for k in range(K // 2)]              # output 2k is fed by the odd network: the switch crosses
    inner = []
    for c in (0, 1):
        sub = [0] * (K // 2)
        for o in range(K):
            if colour[perm[o]] == c:
                sub[o // 2] = perm[o] // 2
        inner.append(_route(sub))
    mid = [[b for pair in zip(a, b_) for b in pair] for a, b_ in zip(*inner)]
    return [first] + mid + [last]


def route(perm: Sequence[int]) -> List[int]:
    perm = [int(p) for p in perm]
    assert sorted(perm) == list(range(len(perm)))
    return [b for layer in _route(perm) for b in layer]


class Switch(NamedTuple):
    j: int
    jp: int
    bit: int                 # what assert_bit's cells hold
    sel: Tuple[int, int]     # what the two selects' sel cells hold
    in_j: List[int]          # the limbs the selects read for position j and for its partner
    in_jp: List[int]
    out_j: List[int]
    out_jp: List[int]


class Trace(NamedTuple):
    layers: List[List[int]]        # every layer's values ([] for K = 1)
    routed: List[int]              # d_i: what the final block of output i multiplies
    r_chains: List[List[P.Step]]   # nr steps each
    finals: List[P.Step]
    mixed: List[int]               # c'_i
    switches: List[List[Switch]]   # per layer, in switch order, limb by limb
    last: List[List[int]]          # the limbs the last layer leaves at every position (K = 1: c_1's)


def mix_trace(n: int, cts: Sequence[int], bits: Sequence[int], rs: Sequence[int], forge=None, limb_bits: int = 64, limbs: int = 0) -> Trace:
    """forge, everything downstream of it recomputed consistently (the soundness negatives):
      ('bit', l, s, 2)   switch s of layer l holds the bit 2: its selects leave in[j] + 2 (in[j'] - in[j]) and the mirror image
      ('dup', l, s)      the switch's two selects run under different bits: one input leaves twice, the other is dropped
      ('src', l, j, 1)   the selects of layer l read, for position j, the previous layer's limb 0 plus 1
      ('in', j, 1)       layer 0 reads c_j + 1 while the assigned (exposed) cells keep c_j
      ('rn', i, 1)       the final block's second operand is rn_i + 1
      ('d', i, 1)        the final block's first operand is d_i + 1
    A position's value is its limbs recomposed (reduced mod n^2 where a forge left it outside)."""
    n2 = n * n
    K = len(cts)
    assert K == len(rs) >= 1
    L = limbs or 2 * -(-n.bit_length() // limb_bits)
    lim = lambda v: P.decompose_biguint(v, L, limb_bits)
    val = lambda ls: sum(x << (limb_bits * t) for t, x in enumerate(ls))
    cur = [lim(int(c)) for c in cts]
    layers, switches, at = [], [], 0
    for l, layer in enumerate(benes_layers(K)):
        nxt, row = [None] * K, []
        for s, (j, jp) in enumerate(layer):
            b = int(bits[at])
            at += 1
            here = lambda name: forge is not None and forge[0] == name and forge[1] == l and forge[2] == s
            if here("bit"):
                b = forge[3]
            sel = (b, 1 - b) if here("dup") else (b, b)
            in_j, in_jp = list(cur[j]), list(cur[jp])
            if forge is not None and ((forge[0] == "src" and forge[1] == l) or (forge[0] == "in" and l == 0)):
                pos, delta = (forge[2], forge[3]) if forge[0] == "src" else (forge[1], forge[2])
                if pos == j:
                    in_j[0] += delta
                if pos == jp:
                    in_jp[0] += delta
            out_j = [(x - y) * sel[0] + y for x, y in zip(in_jp, in_j)]          # select(in[j'], in[j], b)
            out_jp = [(x - y) * sel[1] + y for x, y in zip(in_j, in_jp)]         # select(in[j], in[j'], b)
            nxt[j], nxt[jp] = out_j, out_jp
            row.append(Switch(j, jp, b, sel, in_j, in_jp, out_j, out_jp))
        switches.append(row)
        layers.append([val(ls) for ls in nxt])
        cur = nxt
    assert at == len(bits)
    if K == 1 and forge is not None and forge[0] == "in":
        raise ValueError("one ciphertext has no layer 0")
    routed = [val(ls) % n2 for ls in cur]
    t = Trace(layers, routed, [], [], [], switches, cur)
    for i, (d, r) in enumerate(zip(routed, rs)):
        rn, sr = P.pow_mod_fixed_exp_trace(r, n, n2)
        assert len(sr) == n_steps_r(n)
        hit = forge is not None and forge[0] in ("rn", "d") and forge[1] == i
        fin = P.mul_mod_step(d + forge[2] if hit and forge[0] == "d" else d, rn + forge[2] if hit and forge[0] == "rn" else rn, n2)
        t.r_chains.append(sr)
        t.finals.append(fin)
        t.mixed.append(fin[3])
    return t


def records(trace: Trace) -> List[P.Step]:
    """the records in pz_paillier_mix's order"""
    out: List[P.Step] = []
    for sr, fin in zip(trace.r_chains, trace.finals):
        out += list(sr) + [fin]
    return out


def mix_cells(n: int, cts: Sequence[int], rs: Sequence[int], res: Sequence[int], enc_bits: int, limb_bits: int, lb: int, trace: Trace):
    """the stream of `trace` (mix_trace(.., limb_bits=limb_bits, limbs=2 * enc_bits // limb_bits)).  The assigned cells always hold
    `cts`, `rs` and `res`; a switch's cells hold what the trace's selects read and left.
    -> (advice cells, lookup cells, {name: (advice offset, lookup offset)}) as canonical integers"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    n2 = n * n
    K = len(cts)
    assert len(rs) == len(res) == len(trace.mixed) == K and all(len(ls) == L for ls in trace.last)
    adv: List[int] = []
    lk: List[int] = []
    seg = {}

    def put(name, a, l=()):
        seg.setdefault(name, (len(adv), len(lk)))
        adv.extend(a)
        lk.extend(l)

    put("assign_n", *P.expand_assign_cells(n, Ln, limb_bits, lb))
    for c in cts:
        put("assign_cts", *P.expand_assign_cells(c, L, limb_bits, lb))
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
    seg["network"] = (len(adv), len(lk))
    for row in trace.switches:
        for sw in row:
            put("network", [0, sw.bit, sw.bit, sw.bit])
            for t in range(L):
                put("network", P._select_cells(sw.in_jp[t], sw.in_j[t], sw.sel[0]))
                put("network", P._select_cells(sw.in_j[t], sw.in_jp[t], sw.sel[1]))
    seg["outputs"] = (len(adv), len(lk))
    for sr, fin in zip(trace.r_chains, trace.finals):
        put("outputs", [1, 0])
        for st in sr:
            put("outputs", *P.expand_mul_mod_cells(*st, n2, L, lb, limb_bits))
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


def mix_gate_mask(count: int, enc_bits: int, limb_bits: int, lb: int, n_steps_r_: int) -> np.ndarray:
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
    mm = mask(P.gate_offsets_mul_mod(L, lb, limb_bits))
    parts = [narrow] + [wide] * count + [narrow] * count
    parts.append(mask(P.gate_offsets_square(Ln)))
    parts.append(mask(P.gate_offsets_refresh(P.refresh_aux(limb_bits, Ln, Ln), limb_bits, lb)))
    parts.append(np.zeros(1, dtype=np.uint8))                            # load_zero
    switch = mask(([0] + [4 + 8 * t + o for t in range(2 * L) for o in (0, 4)], 4 + 16 * L))
    parts += [switch] * n_bits(count)
    two = np.zeros(2, dtype=np.uint8)
    parts += [np.concatenate([two] + [mm] * (n_steps_r_ + 1))] * count
    parts += [wide, mask(P.gate_offsets_assert_equal(L))] * count
    return np.concatenate(parts)


def statement(n: int, cts: Sequence[int], mixed: Sequence[int], enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | c_1[2 Ln] | .. | c_K[2 Ln] | c'_1[2 Ln] | .. | c'_K[2 Ln], little-endian limbs"""
    Ln = enc_bits // limb_bits
    out = P.decompose_biguint(n, Ln, limb_bits)
    for v in list(cts) + list(mixed):
        out += P.decompose_biguint(v, 2 * Ln, limb_bits)
    return out
