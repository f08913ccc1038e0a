"""Test-side restatement of the weighted tally circuit (kind 4 / "wtally"), independent of the product: per
ciphertext oracle.pyref.pow_mod_uniform_trace over W weight bits, the product tree of tests.tally_ref over the powers, the cell
stream composed from oracle.pyref's per-operation emitters and its gate mask from the gate_offsets_* functions.  Python integers
throughout.  The product must not import this module.

Record order: the chains' 2 B W records chain-major (chain i, bit j: (acc, sq, q, r) at 2 (i W + j), (sq, sq, q, sq') next), then the
tree's B - 1 records in tally_tree order.  B = 1 has no tree: the root is the power."""
from typing import List, Sequence, Tuple

import numpy as np

from oracle import pyref as P
from tests.tally_ref import check_columns, place, tally_tree  # noqa: F401  (re-exported: the tests take them from here)

R = P.FR_R


def wtally_tree(count: int) -> List[Tuple[int, int]]:
    return tally_tree(count) if count > 1 else []


def wtally_trace(n: int, cts: Sequence[int], weights: Sequence[int], w_bits: int, forge=None):
    """-> (root, chains, tree, powers, exponents): chains[i] = the 2 W steps of chain i, run with exponents[i]; tree = the B - 1 steps
    in tree order.
    forge, everything downstream of it recomputed consistently (the soundness negatives):
      ('weight', i, w')          chain i runs with w' instead of weights[i]
      ('leaf', i, delta)         chain i's first sq is c_i + delta
      ('tree', t, 'a'|'b', delta) tree block t's operand is the honest value + delta"""
    n2 = n * n
    assert len(cts) == len(weights) >= 1
    chains: List[List[P.Step]] = []
    powers: List[int] = []
    exponents: List[int] = []
    for i, (c, w) in enumerate(zip(cts, weights)):
        if forge is not None and forge[0] == "weight" and forge[1] == i:
            w = forge[2]
        if forge is not None and forge[0] == "leaf" and forge[1] == i:
            c = c + forge[2]
        p, st = P.pow_mod_uniform_trace(c, w, w_bits, n2)
        assert len(st) == 2 * w_bits
        chains.append(st)
        powers.append(p)
        exponents.append(w)
    tree: List[P.Step] = []
    for t, (ia, ib) in enumerate(wtally_tree(len(cts))):
        a = powers[-ia - 1] if ia < 0 else tree[ia][3]
        b = powers[-ib - 1] if ib < 0 else tree[ib][3]
        if forge is not None and forge[0] == "tree" and forge[1] == t:
            if forge[2] == "a":
                a += forge[3]
            else:
                b += forge[3]
        tree.append(P.mul_mod_step(a, b, n2))
    root = tree[-1][3] if tree else powers[0]
    return root, chains, tree, powers, exponents


def records(chains: Sequence[Sequence[P.Step]], tree: Sequence[P.Step]) -> List[P.Step]:
    """the records in pz_paillier_wtally's order"""
    return [st for ch in chains for st in ch] + list(tree)


def wtally_cells(n: int, cts: Sequence[int], weights: Sequence[int], res: int, w_bits: int, enc_bits: int, limb_bits: int, lb: int,
                 trace=None):
    """the stream: assign n; assign c_i at full width; load_witness(w_i); square + refresh once; per chain [1, 0], num_to_bits and the W
    (mul_mod, select, square_mod) blocks; the tree's blocks; assign res; assert_equal_fresh(root, res).
    trace = wtally_trace's result to expand (default: the honest one).  The weight cells of step 3 always hold `weights`; a chain's
    num_to_bits holds the exponent its records were run with.
    -> (advice cells, lookup cells, {name: (advice offset, lookup offset)}) as canonical integers"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    n2 = n * n
    if trace is None:
        trace = wtally_trace(n, cts, weights, w_bits)
    root, chains, tree, _, exponents = trace
    assert len(chains) == len(cts) and len(tree) == max(len(cts) - 1, 0)
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
    put("weights", [int(w) for w in weights])
    nl = P.decompose_biguint(n, Ln, limb_bits)
    sq_cells, prod = P._mul_cells(nl, nl, 2 * Ln - 1)
    put("square", sq_cells)
    inc = P.refresh_aux(limb_bits, Ln, Ln)
    assert len(inc) == L
    r_adv, r_lk, fresh = P.expand_refresh_cells(prod, inc, limb_bits, lb)
    assert P.get_biguint(fresh, limb_bits) == n2
    put("refresh", r_adv, r_lk)
    for st, e in zip(chains, exponents):
        put("chains", [1, 0])
        nb_cells, bits = P._num_to_bits_cells(e, w_bits)
        assert len(nb_cells) == 7 * w_bits - 2
        put("chains", nb_cells)
        for j in range(w_bits):
            st_mul, st_sq = st[2 * j], st[2 * j + 1]
            put("chains", *P.expand_mul_mod_cells(*st_mul, n2, L, lb, limb_bits))
            acc_l, mul_l = P.decompose_biguint(st_mul[0], L, limb_bits), P.decompose_biguint(st_mul[3], L, limb_bits)
            for t in range(L):
                put("chains", P._select_cells(mul_l[t], acc_l[t], bits[j]))
            put("chains", *P.expand_mul_mod_cells(*st_sq, n2, L, lb, limb_bits))
    for st in tree:
        put("tree", *P.expand_mul_mod_cells(*st, n2, L, lb, limb_bits))
    seg.setdefault("tree", (len(adv), len(lk)))
    put("assign_res", *P.expand_assign_cells(res, L, limb_bits, lb))
    ae, bit = P.expand_assert_equal_fresh_cells(P.decompose_biguint(root, L, limb_bits), P.decompose_biguint(res, L, limb_bits))
    put("assert_equal", ae)
    seg["end"] = (len(adv), len(lk))
    seg["satisfied"] = bool(bit)
    return [v % R for v in adv], [v % R for v in lk], seg


def wtally_gate_mask(count: int, w_bits: int, enc_bits: int, limb_bits: int, lb: int) -> np.ndarray:
    """uint8 selector over the advice stream (1 where a gate window starts), from the gate_offsets_* functions"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    W = w_bits

    def mask(part):
        g, n = part
        m = np.zeros(n, dtype=np.uint8)
        m[np.asarray(g, dtype=np.int64)] = 1
        return m

    wide = mask(P.gate_offsets_assign(L, limb_bits, lb))
    mm = mask(P.gate_offsets_mul_mod(L, lb, limb_bits))
    parts = [mask(P.gate_offsets_assign(Ln, limb_bits, lb))] + [wide] * count
    parts.append(np.zeros(count, dtype=np.uint8))                      # load_witness: no gate
    parts.append(mask(P.gate_offsets_square(Ln)))
    parts.append(mask(P.gate_offsets_refresh(P.refresh_aux(limb_bits, Ln, Ln), limb_bits, lb)))
    # one chain: [1, 0]; num_to_bits (the inner product's W - 1 windows, then assert_bit per bit); W blocks
    ntb = mask(([3 * i for i in range(W - 1)] + [1 + 3 * (W - 1) + 4 * i for i in range(W)], 7 * W - 2))
    sel = mask(([8 * t + o for t in range(L) for o in (0, 4)], 8 * L))
    chain = np.concatenate([np.zeros(2, dtype=np.uint8), ntb] + [mm, sel, mm] * W)
    parts += [chain] * count
    parts += [mm] * (count - 1)
    parts.append(wide)
    parts.append(mask(P.gate_offsets_assert_equal(L)))
    return np.concatenate(parts)


def statement(n: int, cts: Sequence[int], weights: Sequence[int], c: int, enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | c_1[2 Ln] | .. | c_B[2 Ln] | w_1 | .. | w_B | C[2 Ln], little-endian limbs; a weight is one value"""
    Ln = enc_bits // limb_bits
    out = P.decompose_biguint(n, Ln, limb_bits)
    for v in cts:
        out += P.decompose_biguint(v, 2 * Ln, limb_bits)
    out += [int(w) for w in weights]
    out += P.decompose_biguint(c, 2 * Ln, limb_bits)
    return out
