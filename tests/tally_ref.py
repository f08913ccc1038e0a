"""Test-side restatement of the tally circuit, independent of the product: the product tree over
oracle.pyref.mul_mod_step, the cell stream composed from oracle.pyref's per-operation emitters, its gate mask from the gate_offsets_*
functions, and a column-form satisfiability check.  Python integers throughout.  The product must not import this module.

Tree order: cur = [c_1 .. c_B]; while len(cur) > 1: one mul_mod per neighbouring pair, in order; an odd last element is carried up
without a block.  Records and blocks are numbered as this loop creates them (level-major)."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import pyref as P

R = P.FR_R


def tally_tree(count: int) -> List[Tuple[int, int]]:
    """[(a, b)] per block: an operand >= 0 is the block that produced it, -(1 + i) the ciphertext c_(i+1)"""
    cur = [-(1 + i) for i in range(count)]
    blocks: List[Tuple[int, int]] = []
    while len(cur) > 1:
        nxt = []
        for j in range(len(cur) // 2):
            nxt.append(len(blocks))
            blocks.append((cur[2 * j], cur[2 * j + 1]))
        if len(cur) % 2:
            nxt.append(cur[-1])
        cur = nxt
    return blocks


def tally_trace(n: int, cts: Sequence[int], forge=None):
    """-> (root, [Step]) with the steps in tree order.  forge = (block index, 'a' | 'b', delta): that block's operand is taken as the
    honest value + delta, everything downstream follows from the forged record (the soundness negatives)."""
    n2 = n * n
    steps: List[P.Step] = []
    for t, (ia, ib) in enumerate(tally_tree(len(cts))):
        a = cts[-ia - 1] if ia < 0 else steps[ia][3]
        b = cts[-ib - 1] if ib < 0 else steps[ib][3]
        if forge is not None and forge[0] == t:
            if forge[1] == "a":
                a += forge[2]
            else:
                b += forge[2]
        steps.append(P.mul_mod_step(a, b, n2))
    return steps[-1][3], steps


def tally_cells(n: int, cts: Sequence[int], res: int, enc_bits: int, limb_bits: int, lb: int, steps: Optional[Sequence[P.Step]] = None):
    """the stream of section 1: assign n; assign c_i at full width; square + refresh once; the B - 1 blocks; assign res;
    assert_equal_fresh(root, res).  steps: the records to expand (default: the honest trace).
    -> (advice cells, lookup cells, {name: (advice offset, lookup offset)}) as canonical integers"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    if steps is None:
        _, steps = tally_trace(n, cts)
    assert len(steps) == len(cts) - 1
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
    nl = P.decompose_biguint(n, Ln, limb_bits)
    sq_cells, prod = P._mul_cells(nl, nl, 2 * Ln - 1)
    put("square", sq_cells)
    inc = P.refresh_aux(limb_bits, Ln, Ln)
    assert len(inc) == L
    r_adv, r_lk, fresh = P.expand_refresh_cells(prod, inc, limb_bits, lb)
    assert P.get_biguint(fresh, limb_bits) == n * n
    put("refresh", r_adv, r_lk)
    for st in steps:
        put("tree", *P.expand_mul_mod_cells(*st, n * n, L, lb, limb_bits))
    put("assign_res", *P.expand_assign_cells(res, L, limb_bits, lb))
    ae, bit = P.expand_assert_equal_fresh_cells(P.decompose_biguint(steps[-1][3], L, limb_bits), P.decompose_biguint(res, L, limb_bits))
    put("assert_equal", ae)
    seg["end"] = (len(adv), len(lk))
    seg["satisfied"] = bool(bit)
    return [v % R for v in adv], [v % R for v in lk], seg


def tally_gate_mask(count: int, enc_bits: int, limb_bits: int, lb: int) -> np.ndarray:
    """uint8 selector over the advice stream (1 where a gate window starts), from the gate_offsets_* functions"""
    Ln = enc_bits // limb_bits
    L = 2 * Ln

    def mask(part):
        g, n = part
        m = np.zeros(n, dtype=np.uint8)
        m[np.asarray(g, dtype=np.int64)] = 1
        return m

    wide = mask(P.gate_offsets_assign(L, limb_bits, lb))
    parts = [mask(P.gate_offsets_assign(Ln, limb_bits, lb))] + [wide] * count
    parts.append(mask(P.gate_offsets_square(Ln)))
    parts.append(mask(P.gate_offsets_refresh(P.refresh_aux(limb_bits, Ln, Ln), limb_bits, lb)))
    parts.append(np.tile(mask(P.gate_offsets_mul_mod(L, lb, limb_bits)), count - 1))
    parts.append(wide)
    parts.append(mask(P.gate_offsets_assert_equal(L)))
    return np.concatenate(parts)


def statement(n: int, cts: Sequence[int], c: int, enc_bits: int, limb_bits: int) -> List[int]:
    """n[Ln] | c_1[2 Ln] | .. | c_B[2 Ln] | C[2 Ln], little-endian limbs"""
    Ln = enc_bits // limb_bits
    out = P.decompose_biguint(n, Ln, limb_bits)
    for v in list(cts) + [c]:
        out += P.decompose_biguint(v, 2 * Ln, limb_bits)
    return out


def place(adv: Sequence[int], lk: Sequence[int], starts: Sequence[int], n_adv: int, n_lk: int, max_rows: int, k: int, constants: Sequence[int],
          instances: Optional[Sequence[int]] = None) -> List[List[int]]:
    """the streams in column form: advice by the break points `starts` (a column's last cell is also row 0 of the next), the lookup
    stream cut plainly at max_rows, the constants column, then the instance column if there is one; unfilled rows are 0"""
    n = 1 << k
    cols = [[0] * n for _ in range(n_adv + n_lk + 1 + (1 if instances is not None else 0))]
    starts = [int(s) for s in starts]
    for j in range(n_adv):
        lo, hi = starts[j], starts[j + 1]
        if lo >= len(adv):
            break
        end = min(hi + 1, len(adv))
        cols[j][: end - lo] = adv[lo:end]
    for t in range(0, len(lk), max_rows):
        chunk = lk[t:t + max_rows]
        cols[n_adv + t // max_rows][: len(chunk)] = chunk
    cols[n_adv + n_lk][: len(constants)] = [int(c) % R for c in constants]
    if instances is not None:
        cols[n_adv + n_lk + 1][: len(instances)] = [int(v) % R for v in instances]
    return cols


def check_columns(selectors, map_col, map_row, table, cols, n_lk: int):
    """column-form satisfiability: every enabled gate a + b c = d on rows r .. r + 3 of its advice column; every cell equal to its
    image under the permutation; every cell of the n_lk lookup-advice columns (those after the advice columns) in `table`.
    -> [('gate' | 'copy' | 'lookup', column, row)]"""
    sel = np.asarray(selectors)
    mc, mr = np.asarray(map_col).astype(np.int64), np.asarray(map_row).astype(np.int64)
    A = sel.shape[0]
    bad = []
    for j in range(A):
        col = cols[j]
        for r in np.nonzero(sel[j])[0].tolist():
            if (col[r] + col[r + 1] * col[r + 2] - col[r + 3]) % R:
                bad.append(("gate", j, r))
    for j in range(mc.shape[0]):
        moved = np.nonzero((mc[j] != j) | (mr[j] != np.arange(mc.shape[1])))[0].tolist()
        for r in moved:
            if cols[j][r] != cols[int(mc[j, r])][int(mr[j, r])]:
                bad.append(("copy", j, r))
    tab = table if isinstance(table, (set, frozenset, range)) else set(table)
    for j in range(A, A + n_lk):
        for r, v in enumerate(cols[j]):
            if v not in tab:
                bad.append(("lookup", j, r))
    return bad
