"""The STRUCTURE of the reference's circuits as halo2's keygen sees it -- selector positions, copy constraints, constants, lookup
sources, the break-point column layout -- generated at any size without touching a witness value.

In the reference this is what `keygen_vk` / `keygen_pk` extract by running `synthesize` of halo2-lib's builder over the drivers
(/root/reference/src/bench.rs:33-117 with PaillierChip::{encrypt, add}, src/paillier.rs:32-85; reached from bench.rs:161-175): the
structure is a function of the SHAPE only -- key size, limb width, lookup bits, and the bits of the two fixed exponents
(paillier.rs:50-55 pulls m and n out of the witness, so they shape the circuit).  K4 (csrc/pz_witness.hip) writes the VALUES of the
same cells; this module says which cells are tied together, so that prover.keygen can build the sigma polynomials and the
selectors of the very circuit K4 fills (the connected proof of tests/test_gpu_connected_proof.py and bench.py's with_next_rows).

How: one value-free walk over a single mul_mod block records, per cell, the cell it copies (or which operand limb, or which
constant), the gate windows and the looked-up cells; the circuit's ~6000 identical blocks are that template tiled with numpy, the
operand limbs resolved per step from pow_mod_fixed_exp's schedule.  Equality classes become cycles of sigma by one sort (torch, on
the GPU when there is one: 4 x 10^8 cells at config c2).

The per-primitive patterns restate halo2-lib / biguint-halo2 [D] like K4's: layout parity with the
reference's floating dependency versions is unpinned; tests/test_circuit_structure.py holds this module against the oracle's
independent restatement (oracle/pyref.py::expand_circuit_cells_wired, gate_mask_circuit) cell for cell.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import layout, mix
from .prover import CircuitStructure


class _Walk:
    """records cells in emission order: what each copies, constants, gate windows, lookups.  A cell reference is a global stream
    index (int) or, inside the block template, an operand limb ('a' | 'b' | 'n', j)."""

    def __init__(self, base: int = 0):
        self.base = base
        self.src: List = []        # -1 | int (absolute) | (kind, j)
        self.cval: List = []       # None | int
        self.gates: List[int] = []     # local positions
        self.lk: List = []         # cell references, in lookup-stream order

    def put(self, src=-1) -> int:
        self.src.append(-1 if src is None else src)
        self.cval.append(None)
        return self.base + len(self.src) - 1

    def putc(self, v: int) -> int:
        self.src.append(-1)
        self.cval.append(v)
        return self.base + len(self.src) - 1

    def pair(self, src, copy: int):
        if src is None:
            return
        assert self.src[copy - self.base] == -1
        self.src[copy - self.base] = src

    def gate(self, cell: int):
        self.gates.append(cell - self.base)

    @property
    def n(self) -> int:
        return len(self.src)


def _range_check(w: _Walk, xcell, bits: int, lb: int):
    """RangeChip::range_check: digits + running recomposition, then the top digit's tail gate; -> the cell holding the value"""
    k = -(-bits // lb)
    rem = bits % lb
    last_cell = xcell
    holder = xcell
    if k > 1:
        c0 = w.put()
        w.lk.append(c0)
        w.gate(c0)
        acc_cell = c0
        for gi in range(1, k):
            last_cell = w.put()
            w.lk.append(last_cell)
            w.putc(1 << (lb * gi))
            acc_cell = w.put()
            if gi < k - 1:
                w.gate(acc_cell)
        w.pair(xcell, acc_cell)
        holder = acc_cell
    else:
        w.lk.append(xcell)
    if rem == 1:
        z = w.putc(0)
        w.gate(z)
        w.put(last_cell); w.put(last_cell); w.put(last_cell)
    elif rem > 1:
        z = w.putc(0)
        w.gate(z)
        w.put(last_cell); w.putc(1 << (lb - rem)); w.lk.append(w.put())
    return holder


def _assign(w: _Walk, nl: int, limb_bits: int, lb: int) -> List[int]:
    cells = [w.put() for _ in range(nl)]
    for c in cells:
        _range_check(w, c, limb_bits, lb)
    return cells


def _mul_cells(w: _Walk, xs: Sequence, ys: Sequence, D: int) -> List[int]:
    zc = w.putc(0)
    xe = list(xs) + [zc] * (D - len(xs))
    ye = list(ys) + [zc] * (D - len(ys))
    prod = []
    for i in range(D):
        z = w.putc(0)
        w.gate(z)
        cell = None
        for j in range(i + 1):
            w.put(xe[j]); w.put(ye[i - j])
            cell = w.put()
            if j < i:
                w.gate(cell)
        prod.append(cell)
    return prod


def _is_equal(w: _Walk, xc, yc) -> None:
    c_d = w.put()
    w.gate(c_d)
    w.put(yc); w.putc(1); w.put(xc)
    c_z = w.put()
    w.gate(c_z)
    c_a = w.put(c_d)
    w.put(); w.putc(1)
    z2 = w.putc(0)
    w.gate(z2)
    w.put(c_a); w.put(c_z); w.putc(0)


def _div_mod(w: _Walk, vcell, limb_bits: int) -> Tuple[int, int]:
    c_qd = w.put()
    c_rd = w.put()
    z = w.putc(0)
    w.gate(z)
    w.put(c_qd); w.putc(1 << limb_bits)
    c_pr = w.put()
    d = w.put()
    w.gate(d)
    w.put(c_pr); w.putc(1); w.put(vcell)
    _is_equal(w, c_rd, None)
    return c_qd, c_rd


def _mul_mod(w: _Walk, a: Sequence, b: Sequence, nfresh: Sequence, L: int, limb_bits: int, lb: int) -> List[int]:
    """BigUintChip::mul_mod: assign q, n, r; the two limb convolutions; qn + r; is_equal_muled's carry chain; r < n.  -> r's cells"""
    ql = _assign(w, L, limb_bits, lb)
    nl = _assign(w, L, limb_bits, lb)
    rl = _assign(w, L, limb_bits, lb)
    for c, srcn in zip(nl, nfresh):
        w.pair(srcn, c)
    D = 2 * L - 1
    p_ab = _mul_cells(w, a, b, D)
    p_qn = _mul_cells(w, ql, nl, D)
    qnr = list(p_qn)
    for i in range(L):
        g = w.put(p_qn[i])
        w.gate(g)
        w.putc(1); w.put(rl[i])
        qnr[i] = w.put()
    m = (1 << limb_bits) - 1
    MAX = L * m * m + m
    cb = (2 * MAX).bit_length() - limb_bits
    c_zero = w.putc(0)
    c_one = w.putc(1)
    carry, accx, eq_cell = c_zero, c_zero, c_one
    for i in range(D):
        c_diff = w.put()
        w.gate(c_diff)
        w.put(qnr[i]); w.putc(1); w.put(p_ab[i])
        g = w.put(c_diff)
        w.gate(g)
        w.put(carry); w.putc(1)
        s1 = w.put()
        w.gate(s1)
        w.putc(MAX); w.putc(1)
        c_s = w.put()
        new_carry, cmod = _div_mod(w, c_s, limb_bits)
        g = w.put(accx)
        w.gate(g)
        w.putc(1); w.putc(MAX)
        c_t = w.put()
        q_acc, mod_acc = _div_mod(w, c_t, limb_bits)
        _is_equal(w, cmod, mod_acc)
        g = w.putc(0)
        w.gate(g)
        w.put(eq_cell); w.put()
        eq_cell = w.put()
        accx = q_acc
        if i < D - 1:
            _range_check(w, new_carry, cb, lb)
        else:
            _is_equal(w, new_carry, accx)
            g = w.putc(0)
            w.gate(g)
            w.put(eq_cell); w.put()
            eq_cell = w.put()
        carry = new_carry
    borrow = c_zero
    for i in range(L):
        g = w.put(nl[i])
        w.gate(g)
        w.putc(1); w.put(borrow); w.put()
        w.put()
        c_lt = w.put()
        c_out = w.put()
        g = w.put(rl[i])
        w.gate(g)
        w.put(c_lt); w.putc(1 << limb_bits); w.put()
        _range_check(w, c_out, limb_bits, lb)
        borrow = c_lt
    w.put(borrow)
    return rl


@dataclass
class _Template:
    cells: int
    self_or_local: np.ndarray        # int64 [cells]: local source index, or the cell's own index
    ext: Dict[str, Tuple[np.ndarray, np.ndarray]]   # kind -> (positions, limb index)
    const_pos: np.ndarray            # positions of constant cells
    const_val: List[int]             # their values
    gates: np.ndarray
    lk: np.ndarray                   # local positions, lookup-stream order
    r_cells: np.ndarray              # local positions of r's limb cells


def _make_template(w: _Walk, outs: List[int]) -> _Template:
    """a finished template walk -> arrays; outs: the local positions of the block's outputs"""
    n = w.n
    sol = np.arange(n, dtype=np.int64)
    ext: Dict[str, Tuple[List[int], List[int]]] = {"a": ([], []), "b": ([], []), "n": ([], []), "s": ([], [])}
    for i, s in enumerate(w.src):
        if isinstance(s, tuple):
            ext[s[0]][0].append(i)
            ext[s[0]][1].append(s[1])
        elif s >= 0:
            sol[i] = s
    cpos = [i for i, v in enumerate(w.cval) if v is not None]
    assert all(isinstance(c, int) for c in w.lk)
    return _Template(n, sol, {k: (np.asarray(p, dtype=np.int64), np.asarray(j, dtype=np.int64)) for k, (p, j) in ext.items()},
                     np.asarray(cpos, dtype=np.int64), [w.cval[i] for i in cpos], np.asarray(w.gates, dtype=np.int64),
                     np.asarray(w.lk, dtype=np.int64), np.asarray(outs, dtype=np.int64))


def _block_template(L: int, limb_bits: int, lb: int) -> _Template:
    w = _Walk()
    A = [("a", j) for j in range(L)]
    B = [("b", j) for j in range(L)]
    Nf = [("n", j) for j in range(L)]
    return _make_template(w, _mul_mod(w, A, B, Nf, L, limb_bits, lb))


def _uniform_template(L: int, limb_bits: int, lb: int) -> _Template:
    """one exponent bit of the uniform-shape circuit (pz_paillier_encrypt_uniform, circuit kind 2): mul_mod(acc, sq), the limb-wise
    select(bit, product, acc) = 8 cells per limb [d | 1 | acc | prod | acc | bit | d | out] with gates at 0 and 4, square_mod(sq).
    Operand limbs: 'a' = acc, 'b' = sq, 'n' = the refreshed n^2, 's' = the bit's cell.  r_cells holds the NEW acc (select outputs)
    then the NEW sq (the square's remainder), L cells each."""
    w = _Walk()
    A = [("a", j) for j in range(L)]
    B = [("b", j) for j in range(L)]
    Nf = [("n", j) for j in range(L)]
    mul = _mul_mod(w, A, B, Nf, L, limb_bits, lb)
    outs = []
    for t in range(L):
        c_d = w.put()
        w.gate(c_d)
        w.putc(1); w.put(("a", t)); w.put(mul[t])
        g = w.put(("a", t))
        w.gate(g)
        w.put(("s", 0)); w.put(c_d)
        outs.append(w.put())
    return _make_template(w, outs + _mul_mod(w, B, B, Nf, L, limb_bits, lb))


@dataclass
class StructureArrays:
    """stream-level structure: everything indexed by the advice stream's cell index"""
    n_cells: int
    src: np.ndarray              # int64 [n_cells]: the advice cell each cell copies (itself if none); constants point at -(1 + const id)
    gate_mask: np.ndarray        # uint8 [n_cells]
    lookup_src: np.ndarray       # int64 [n_lookups]
    constants: List[int]         # distinct constants in order of first use
    result_cell: int
    n_steps_g: int
    n_steps_r: int
    # stream indices of the cells a circuit with the instance column exposes, in the column's row order: the limb cells of
    # n | g | c (encrypt, encrypt_uniform), n | g | m | c (decrypt), n | g | c1 | c2 | c (add), n | c_1 | .. | c_B | C (tally) or n | c_1 | .. | c_B | w_1 | .. |
    # w_B | C (wtally: a weight is ONE cell) -- pz_circuit_public_cells gives the same list -- or n | g | c_1 | .. | c_K | S (ballot: S is
    # the sum's last cell, present for K >= 2; pz_ballot_public_cells) -- or n | v | h | c_1 | u_1 | .. | c_K | u_K (partial;
    # pz_partial_public_cells) -- or n | c_1 | .. | c_K | c'_1 | .. | c'_K (mix; pz_mix_public_cells) -- or n | g | hs | c_1 | .. | c_K | S
    # (sballot; pz_sballot_public_cells) -- or n | hs | c_1 | .. | c_K | c'_1 | .. | c'_K (smix; pz_smix_public_cells) -- or
    # n | hs | G_0 | .. | G_{K-1} | c_1 | .. | c_R | S_1 | .. | S_R (pballot; pz_pballot_public_cells)
    public_cells: Optional[np.ndarray] = None


def _exp_bits(e: int) -> List[int]:
    return [(e >> i) & 1 for i in range(e.bit_length())]


def _flex_sum(w: _Walk, cells: Sequence[int]):
    """FlexGate::sum: m_1 | 1 | m_2 | s_2 | 1 | m_3 | s_3 | ..; a window every 3 cells, the operands copies of the cells above
    -> the last sum's cell (fewer than two cells: nothing is emitted, None)"""
    if len(cells) < 2:
        return None
    sum_c = w.put(cells[0])
    for c in cells[1:]:
        w.gate(sum_c)
        w.putc(1)
        w.put(c)
        sum_c = w.put()
    return sum_c


class _Stream:
    """The advice stream as a sequence of parts, and the shared parts every circuit kind's stream is composed of (stream_structure
    below; the same names in csrc/pz_structure.hip).  The stream's end `off` is where the next part starts: every part is appended
    there.  dev: None -> numpy; a torch device -> the templates are tiled THERE."""

    def __init__(self, L: int, limb_bits: int, lb: int, dev):
        self.L, self.W, self.lb, self.dev = L, limb_bits, lb, dev
        self.off = 0
        self.src: List = []
        self.mask: List[np.ndarray] = []
        self.lk: List = []
        self.const_id: Dict[int, int] = {}
        self.constants: List[int] = []
        self.fresh: Optional[np.ndarray] = None      # the limb cells of the refreshed n^2 (set behind the prefix)
        self.tmpls: List = [_block_template(L, limb_bits, lb)]
        self.bound: List = []                        # per template: (the constant id per const_pos entry, the gate mask)

    def cid(self, v: int) -> int:
        if v not in self.const_id:
            self.const_id[v] = len(self.constants)
            self.constants.append(v)
        return self.const_id[v]

    def open(self) -> _Walk:
        return _Walk(self.off)

    def flush(self, walk: _Walk) -> None:
        """a finished Python-walked part -> arrays"""
        n = walk.n
        s = np.arange(walk.base, walk.base + n, dtype=np.int64)
        for i, v in enumerate(walk.src):
            if v != -1:
                s[i] = v
        for i, v in enumerate(walk.cval):
            if v is not None:
                s[i] = -(1 + self.cid(v))
        mk = np.zeros(n, dtype=np.uint8)
        mk[np.asarray(walk.gates, dtype=np.int64)] = 1
        self.src.append(s)
        self.mask.append(mk)
        self.lk.append(np.asarray(walk.lk, dtype=np.int64))
        self.off = walk.base + n

    def bind_template_constants(self, t: int) -> None:
        T = self.tmpls[t]
        mask = np.zeros(T.cells, dtype=np.uint8)
        mask[T.gates] = 1
        assert len(self.bound) == t
        self.bound.append((np.asarray([self.cid(v) for v in T.const_val], dtype=np.int64), mask))

    def tile(self, bases: np.ndarray, sol: np.ndarray, assigns=()):
        """flattened [len(bases)][len(sol)] array of bases[i] + sol[j], columns `pos` overwritten by `vals` ([ns][len(pos)] or [len(pos)])"""
        if self.dev is None:
            t_ = bases[:, None] + sol[None, :]
            for pos, vals in assigns:
                t_[:, pos] = vals
            return t_.reshape(-1)
        import torch

        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int64).to(self.dev)
        t_ = up(bases)[:, None] + up(sol)[None, :]
        for pos, vals in assigns:
            v = up(vals)
            t_[:, up(pos)] = v if v.dim() == 2 else v[None, :].expand(t_.shape[0], -1)
        return t_.reshape(-1)

    def blocks(self, t: int, a_cells: np.ndarray, b_cells: np.ndarray, s_cells: Optional[np.ndarray] = None) -> np.ndarray:
        """ns blocks of template t at the stream's end; a_cells / b_cells: int64 [ns][L] global cells of the operands' limbs, s_cells:
        [ns] the bit's cell (uniform) -> int64 [ns][..] the global cells of every block's outputs"""
        T = self.tmpls[t]
        const_ids, mask = self.bound[t]
        ns = a_cells.shape[0]
        bases = self.off + T.cells * np.arange(ns, dtype=np.int64)
        assigns = []
        for kind_, cells_ in (("a", a_cells), ("b", b_cells)):
            pos, j = T.ext[kind_]
            assigns.append((pos, cells_[:, j]))
        pos, j = T.ext["n"]
        assigns.append((pos, self.fresh[j]))
        if s_cells is not None:
            pos, _ = T.ext["s"]
            assigns.append((pos, np.repeat(s_cells[:, None], len(pos), axis=1)))
        assigns.append((T.const_pos, -(1 + const_ids)))
        self.src.append(self.tile(bases, T.self_or_local, assigns))
        self.mask.append(np.tile(mask, ns))
        self.lk.append(self.tile(bases, T.lk))
        self.off += ns * T.cells
        return bases[:, None] + T.r_cells[None, :]

    def uniform(self) -> None:
        """the uniform template (template 1) of a circuit with in-circuit bits: added once, its constants bound"""
        if len(self.tmpls) > 1:
            return
        self.tmpls.append(_uniform_template(self.L, self.W, self.lb))
        self.bind_template_constants(1)

    def head(self, w: _Walk) -> np.ndarray:
        """a chain's head in the open walk: assign_constant(1), load_zero -> the initial acc cells [one, zero, ..]"""
        one = w.putc(1)
        z2 = w.putc(0)
        return np.asarray([one] + [z2] * (self.L - 1), dtype=np.int64)

    def bit_chain(self, wb: _Walk, word_cell: int, nbits: int, acc: np.ndarray, sq: np.ndarray):
        """num_to_bits(word_cell, nbits) behind what the open walk wb holds, flushed, then nbits blocks of the uniform template chained
        through acc (select outputs) and sq (square remainders) -> (the last acc cells, the last sq cells)"""
        L, ut = self.L, self.tmpls[1]
        bit_cells = [wb.put()]
        if nbits > 1:
            wb.gate(bit_cells[0])
        acc_cell = bit_cells[0]
        for i in range(1, nbits):
            bit_cells.append(wb.put())
            wb.putc(1 << i)
            acc_cell = wb.put()
            if i < nbits - 1:
                wb.gate(acc_cell)
        wb.pair(word_cell, acc_cell)        # (nbits = 1: the accumulator IS the bit)
        for bc in bit_cells:
            g_ = wb.putc(0)
            wb.gate(g_)
            wb.put(bc); wb.put(bc); wb.put(bc)
        self.flush(wb)
        outs = self.off + ut.cells * np.arange(nbits, dtype=np.int64)[:, None] + ut.r_cells[None, :]
        a_cells = np.concatenate([np.asarray(acc, dtype=np.int64)[None, :], outs[:-1, :L]])
        b_cells = np.concatenate([np.asarray(sq, dtype=np.int64)[None, :], outs[:-1, L:]])
        self.blocks(1, a_cells, b_cells, np.asarray(bit_cells, dtype=np.int64))
        return outs[-1, :L], outs[-1, L:]

    def limb_chain(self, base_cells, limb_cells, n_limbs: int) -> np.ndarray:
        """pow_mod(base, e) over the n_limbs limb cells of an assigned e: the head as a part of its own, then per limb num_to_bits of
        ITS cell and limb_bits uniform blocks -> the power's cells (the last select's outputs)"""
        wc = self.open()
        acc, sq = self.head(wc), base_cells
        self.flush(wc)
        for li in range(n_limbs):
            acc, sq = self.bit_chain(self.open(), limb_cells[li], self.W, acc, sq)
        return acc

    def word_chain(self, word_cell: int, nbits: int, base_cells) -> np.ndarray:
        """pow_mod(base, e) over the nbits bits of a one-cell e: the head and num_to_bits in ONE walk, then nbits uniform blocks
        -> the power's cells"""
        wb = self.open()
        return self.bit_chain(wb, word_cell, nbits, self.head(wb), base_cells)[0]

    def mul_blocks(self, a_blk, b_blk, outer) -> np.ndarray:
        """mul_mod blocks from WHICH block produced each operand: a_blk / b_blk[q] >= 0 names a block of this run (its remainder), the
        entry -(1 + i) the cells outer[i] from outside the run (no block: no part) -> the table of cells that both kinds of entry index"""
        ns = len(a_blk)
        r_of = self.off + self.tmpls[0].cells * np.arange(ns, dtype=np.int64)[:, None] + self.tmpls[0].r_cells[None, :]
        table = np.concatenate([r_of, np.asarray(outer[::-1], dtype=np.int64).reshape(-1, self.L)])
        if ns:
            self.blocks(0, table[np.asarray(a_blk, dtype=np.int64)], table[np.asarray(b_blk, dtype=np.int64)])
        return table

    def mul_block(self, a, b) -> np.ndarray:
        """one mul_mod(a, b) -> r's cells"""
        return self.blocks(0, np.asarray(a, dtype=np.int64)[None, :], np.asarray(b, dtype=np.int64)[None, :])[0]

    def fixed_chain(self, base_cells, e: int):
        """pow_mod_fixed_exp(base, e): the head, then per bit of e the squaring step (cur, cur) and on a set bit (acc, cur): block -1 is
        the base, block -2 the head -> (the power's cells, the number of blocks)"""
        wc = self.open()
        one = self.head(wc)
        self.flush(wc)
        a_blk, b_blk = [], []
        sq_blk, acc_blk = -1, -2
        for bit in _exp_bits(e):
            cur_blk, sq_blk = sq_blk, len(a_blk)
            a_blk.append(cur_blk); b_blk.append(cur_blk)
            if bit:
                a_blk.append(acc_blk); b_blk.append(cur_blk)
                acc_blk = len(a_blk) - 1
        return self.mul_blocks(a_blk, b_blk, [base_cells, one])[acc_blk], len(a_blk)

    def product_tree(self, leaves, tree):
        """the product of the leaves in the order of `tree` (layout.tally_tree: level by level the neighbours of the current list, an odd
        last element carried up; blocks numbered level-major, leaf i is entry -(1 + i)) -> (the root's cells -- one leaf: no block,
        the leaf --, the number of blocks)"""
        nb = len(tree)
        table = self.mul_blocks([t[0] for t in tree], [t[1] for t in tree], leaves)
        return table[nb - 1], nb                  # the root is the last block

    def network(self, ins):
        """the Benes network of mix.py over `ins` as ONE walked part, layer by layer and switch by switch: assert_bit of the switch's own
        bit cell ([0, b, b, b]: the first b is the bit's home, the other two copy it), then per limb select(in[j'], in[j], b) and
        select(in[j], in[j'], b) -- 8 cells each [d | 1 | y | x | y | b | d | out], windows at 0 and 4.  The operands are the previous
        layer's out cells (layer 0: `ins`); values stay in place -> the outputs' cells"""
        count = len(ins)
        wn = self.open()

        def select(x, y, s):
            c_d = wn.put()
            wn.gate(c_d)
            wn.putc(1); wn.put(y); wn.put(x)
            g_ = wn.put(y)
            wn.gate(g_)
            wn.put(s); wn.put(c_d)
            return wn.put()

        cur_c = [list(c) for c in ins]
        for beta in mix.layer_bits(count):
            nxt_c = [None] * count
            for j in range(count):
                if j >> beta & 1:
                    continue
                jp = j | (1 << beta)
                g_ = wn.putc(0)
                wn.gate(g_)
                b_c = wn.put()
                wn.put(b_c); wn.put(b_c)
                lo_c, hi_c = [], []
                for t_ in range(self.L):
                    lo_c.append(select(cur_c[jp][t_], cur_c[j][t_], b_c))
                    hi_c.append(select(cur_c[j][t_], cur_c[jp][t_], b_c))
                nxt_c[j], nxt_c[jp] = lo_c, hi_c
            cur_c = nxt_c
        self.flush(wn)
        return cur_c


def stream_structure(kind: str, enc_bits: int, limb_bits: int, lb: int, exp_g: int = 0, exp_r: int = 0, device: Optional[str] = None,
                     count: Optional[int] = None, w_bits: Optional[int] = None, m_bits: Optional[int] = None,
                     s_limbs: Optional[int] = None, slots: Optional[int] = None) -> StructureArrays:
    """kind 'encrypt': exp_g = the message m, exp_r = the modulus n -- only their BITS are used, as in the reference's circuit
    (pow_mod_fixed_exp, paillier.rs:50-55); kind 'add': no exponents; kind 'encrypt_uniform' (the uniform-shape circuit, SURVEY 8f rank
    4): exp_g is ignored -- the message's bits are witness cells, ONE structure serves every message of a key; kind 'tally': count = B
    full-width ciphertexts multiplied in layout.tally_tree's order, no exponents -- the shape is B and the key
    size alone; kind 'wtally': count = B full-width ciphertexts, each raised to a w_bits-bit weight held in ONE witness cell (pow_mod
    over in-circuit bits, the uniform circuit's block), the powers multiplied in layout.wtally_tree's order
    -- the shape is B, w_bits and the key size alone; kind 'decrypt': 'encrypt_uniform' with the message's limb cells exposed between
    g's and the result's (the statement n | g | m | c); kind 'ballot' (circuit kind 6):
    count = K ciphertexts under one key, each message ONE witness cell decomposed into m_bits in-circuit bits (the uniform circuit's
    block), exp_r = the modulus n (its bits shape every r^n chain), for K >= 2 the sum of the messages -- the shape is K, m_bits and n;
    kind 'partial' (circuit kind 7): count = K ciphertexts one trustee opens under ONE share theta, an
    assign_integer of 2 Ln limbs every chain decomposes (kind 2's pow_mod walk over all its limbs) -- the shape is K and the key size;
    kind 'mix' (circuit kind 8): count = K = 2^d ciphertexts go through the Benes network of mix.py (per switch
    assert_bit of a fresh bit cell, then per limb the two selects under it) and leave as d_i r_i^n mod n^2, exp_r = the modulus n (its
    bits shape every r^n chain) -- the shape is K and n;
    kind 'sballot' (circuit kind 9): count = K short-randomness ballots c_i = g^m_i hs^s_i under one key, each
    message ONE witness cell decomposed into m_bits in-circuit bits as in 'ballot', each s_i an assign_integer of s_limbs limbs that its
    chain decomposes limb by limb ('partial's walk) from the ONE base hs, for K >= 2 the sum of the messages -- no exponent is taken:
    the shape is K, m_bits, s_limbs and the key size, so ONE structure serves every key of a size;
    kind 'smix' (circuit kind 10): count = K = 2^d ciphertexts go through 'mix's network and leave as d_i
    hs^s_i mod n^2, each s_i an assign_integer of s_limbs limbs that its chain decomposes limb by limb ('sballot's hs-chain walk) from
    the ONE base hs -- no exponent is taken: the shape is K, s_limbs and the key size;
    kind 'pballot' (circuit kind 11): count = R packed ballots c_i = (prod_j G_j^v_ij) hs^s_i of slots = K values
    each, every value ONE witness cell decomposed into m_bits in-circuit bits whose chain starts from the limb cells of ITS slot's base
    G_j (an assign_integer at full width, shared by all R ciphertexts), each s_i as in 'sballot', the K powers and hs^s_i folded by K
    blocks, for K >= 2 one sum per ciphertext -- neither an exponent nor the slot width is taken: the shape is R, K, m_bits, s_limbs and
    the key size.
    device: None -> numpy arrays; a torch device ("cuda") -> the template is tiled THERE and `src` / `lookup_src` are tensors on it (at
    config c2 the tiled arrays are 3.2 GB: 0.9 s of host numpy against a few ms; `columns` takes either)."""
    dev = None
    if device is not None:
        import torch

        dev = torch.device(device)

    Ln = enc_bits // limb_bits
    L = 2 * Ln
    if kind not in ("encrypt", "encrypt_uniform", "add", "tally", "wtally", "decrypt", "ballot", "partial", "mix", "sballot", "smix",
                    "pballot"):
        raise ValueError(f"unknown circuit kind {kind!r}")
    # 'decrypt' (circuit kind 5) is the uniform-shape circuit cell for cell: the exposed list alone differs
    statement, kind = kind, ("encrypt_uniform" if kind == "decrypt" else kind)
    if (kind in ("tally", "wtally", "ballot", "partial", "mix", "sballot", "smix", "pballot")) != (count is not None):
        raise ValueError("count belongs to kinds 'tally', 'wtally', 'ballot', 'partial', 'mix', 'sballot', 'smix' and 'pballot', which need it")
    if kind in ("mix", "smix"):
        if not mix.is_count(count):
            raise ValueError(f"a mix takes count = 1, 2, 4 .. {mix.MIX_MAX} ciphertexts, not {count}")
        if kind == "mix" and exp_r < 1:
            raise ValueError("a mix's structure needs exp_r = the modulus n")
    if kind == "partial" and not 1 <= count <= layout.PARTIAL_MAX:
        raise ValueError(f"a trustee opens count = 1 .. {layout.PARTIAL_MAX} ciphertexts in one proof, not {count}")
    if (kind in ("ballot", "sballot", "pballot")) != (m_bits is not None):
        raise ValueError("m_bits belongs to kinds 'ballot', 'sballot' and 'pballot', which need it")
    if (kind in ("sballot", "smix", "pballot")) != (s_limbs is not None):
        raise ValueError("s_limbs belongs to kinds 'sballot', 'smix' and 'pballot', which need it")
    if kind in ("sballot", "smix", "pballot") and not 1 <= s_limbs <= L:
        raise ValueError(f"a short-randomness exponent has s_limbs = 1 .. {L} limbs, not {s_limbs}")
    if (kind == "pballot") != (slots is not None):
        raise ValueError("slots belongs to kind 'pballot', which needs it")
    if kind == "pballot" and not (1 <= slots <= layout.PBALLOT_MAX_SLOTS and count * slots <= layout.BALLOT_MAX):
        raise ValueError(f"a packed ballot has slots = 1 .. {layout.PBALLOT_MAX_SLOTS} with count * slots <= {layout.BALLOT_MAX}, not {slots}")
    if kind in ("ballot", "sballot", "pballot"):
        if not 1 <= count <= layout.BALLOT_MAX:
            raise ValueError(f"a ballot takes count = 1 .. {layout.BALLOT_MAX} ciphertexts, not {count}")
        if not 1 <= m_bits <= layout.BALLOT_MAX_BITS:
            raise ValueError(f"a ballot's message has m_bits = 1 .. {layout.BALLOT_MAX_BITS} bits, not {m_bits}")
        if kind == "ballot" and exp_r < 1:
            raise ValueError("a ballot's structure needs exp_r = the modulus n")
    if (kind == "wtally") != (w_bits is not None):
        raise ValueError("w_bits belongs to kind 'wtally', which needs it")
    if kind == "wtally" and not 1 <= w_bits <= layout.WTALLY_MAX_BITS:
        raise ValueError(f"a weight has w_bits = 1 .. {layout.WTALLY_MAX_BITS} bits, not {w_bits}")
    tree = layout.tally_tree(count) if kind == "tally" else None      # (refuses a count outside 2 .. TALLY_MAX)
    if kind == "wtally":
        tree = layout.wtally_tree(count)                              # (1 .. TALLY_MAX; one ciphertext has no tree)
    # ---- prefix: the four assign_integer (tally: n, then the B ciphertexts at full width), square, refresh, load_zero (not in a
    # tally: nothing is extended there); global indices from 0
    S = _Stream(L, limb_bits, lb, dev)
    w = S.open()
    n_c = _assign(w, Ln, limb_bits, lb)
    if kind in ("tally", "wtally"):
        ct_c = [_assign(w, L, limb_bits, lb) for _ in range(count)]
        g_c = x_c = y_c = []
        wt_c = [w.put() for _ in range(count)] if kind == "wtally" else []     # load_witness(w_i): one cell each, no gate
    elif kind == "partial":
        v_c = _assign(w, L, limb_bits, lb)
        th_c = _assign(w, L, limb_bits, lb)
        ct_c = [_assign(w, L, limb_bits, lb) for _ in range(count)]
    elif kind in ("mix", "smix"):
        hs_c = _assign(w, L, limb_bits, lb) if kind == "smix" else []           # hs: the key's second base, full width
        ct_c = [_assign(w, L, limb_bits, lb) for _ in range(count)]
        rs_c = [_assign(w, s_limbs if kind == "smix" else Ln, limb_bits, lb) for _ in range(count)]      # r_i; 'smix': s_i
    elif kind == "pballot":
        hs_c = _assign(w, L, limb_bits, lb)                                     # hs, then the slot bases G_j: all at full width
        gs_c = [_assign(w, L, limb_bits, lb) for _ in range(slots)]
        vs_c = [[w.put() for _ in range(slots)] for _ in range(count)]          # load_witness(v_ij): one cell each, ciphertext-major
        sums_c = [_flex_sum(w, vs_c[i]) for i in range(count)] if slots >= 2 else []   # over the ciphertext's own values
        rs_c = [_assign(w, s_limbs, limb_bits, lb) for _ in range(count)]       # s_i
    elif kind in ("ballot", "sballot"):
        g_c = _assign(w, Ln, limb_bits, lb)
        hs_c = _assign(w, L, limb_bits, lb) if kind == "sballot" else []        # hs: the key's second base, full width
        ms_c = [w.put() for _ in range(count)]                                 # load_witness(m_i): one cell each, no gate
        sum_c = _flex_sum(w, ms_c)                                             # (count >= 2)
        rs_c = [_assign(w, s_limbs if kind == "sballot" else Ln, limb_bits, lb) for _ in range(count)]   # r_i; 'sballot': s_i
    else:
        g_c = _assign(w, Ln, limb_bits, lb)
        x_c = _assign(w, Ln, limb_bits, lb)
        y_c = _assign(w, Ln, limb_bits, lb)
    prod = _mul_cells(w, n_c, n_c, 2 * Ln - 1)
    inc = layout.refresh_aux(limb_bits, Ln, Ln)
    w.putc(0)
    cur: List = list(prod) + [None] * (len(inc) - len(prod))
    for i in range(len(inc)):
        limb = cur[i]
        for j in range(inc[i] + 1):
            qd, rd = _div_mod(w, limb, limb_bits)
            if j == 0:
                cur[i] = rd
            else:
                g = w.put(cur[i + j])
                w.gate(g)
                w.putc(1); w.put(rd)
                cur[i + j] = w.put()
            limb = qd
    fresh = []
    for c in cur:
        holder = _range_check(w, c, limb_bits, lb)
        fresh.append(c if c is not None else holder)
    S.fresh = np.asarray(fresh, dtype=np.int64)
    zero = w.putc(0) if kind not in ("tally", "wtally") else None
    ext_l = lambda limbs: list(limbs) + [zero] * (L - len(limbs))
    S.flush(w)
    S.bind_template_constants(0)
    if kind in ("encrypt_uniform", "wtally", "ballot", "partial", "sballot", "smix", "pballot"):
        S.uniform()                                                   # the kinds with in-circuit bits

    # ---- the kind's own blocks -> the cells holding its result(s)
    n_steps = [0, 0]
    hs_chain = lambda i: S.limb_chain(hs_c, rs_c[i], s_limbs)         # pow_mod(hs, s_i): every chain from the SAME hs cells
    if kind in ("encrypt", "encrypt_uniform", "add"):
        gm, rn = ext_l(x_c), ext_l(y_c)                               # ('add': the two ciphertexts)
        if kind == "encrypt_uniform":     # g^m over ALL enc_bits bits of m IN the circuit: the same shape for every message
            gm, n_steps[0] = S.limb_chain(ext_l(g_c), x_c, Ln), 2 * Ln * limb_bits
        elif kind == "encrypt":
            gm, n_steps[0] = S.fixed_chain(ext_l(g_c), exp_g)
        if kind != "add":
            rn, n_steps[1] = S.fixed_chain(ext_l(y_c), exp_r)
        roots = [S.mul_block(gm, rn)]
    elif kind == "tally":
        root, n_steps[0] = S.product_tree(ct_c, tree)
        roots = [root]
    elif kind == "wtally":
        powers = [S.word_chain(wt_c[i], w_bits, ct_c[i]) for i in range(count)]
        n_steps[0] = 2 * count * w_bits
        root, n_steps[1] = S.product_tree(powers, tree)
        roots = [root]
    elif kind == "ballot":
        roots = []
        for i in range(count):
            gm = S.word_chain(ms_c[i], m_bits, ext_l(g_c))
            rn, n_steps[1] = S.fixed_chain(ext_l(rs_c[i]), exp_r)
            roots.append(S.mul_block(gm, rn))
        n_steps[0] = 2 * m_bits
    elif kind == "partial":
        roots = [S.limb_chain(v_c, th_c, L)]                          # h = v^theta: every chain decomposes the SAME limb cells of theta
        for j in range(count):
            roots.append(S.limb_chain(S.mul_block(ct_c[j], ct_c[j]), th_c, L))      # from s_j = c_j^2
        n_steps[0] = 2 * L * limb_bits
    elif kind in ("mix", "smix"):
        d_c = S.network(ct_c)
        roots = []
        for i in range(count):
            if kind == "mix":
                rn, n_steps[1] = S.fixed_chain(ext_l(rs_c[i]), exp_r)
            else:
                rn = hs_chain(i)
            roots.append(S.mul_block(d_c[i], rn))
        if kind == "smix":
            n_steps[1] = 2 * s_limbs * limb_bits
    elif kind == "sballot":
        roots = []
        for i in range(count):
            gm = S.word_chain(ms_c[i], m_bits, ext_l(g_c))
            roots.append(S.mul_block(gm, hs_chain(i)))
        n_steps[0], n_steps[1] = 2 * m_bits, 2 * s_limbs * limb_bits
    else:                                                             # 'pballot'
        roots = []
        for i in range(count):
            powers = [S.word_chain(vs_c[i][j], m_bits, gs_c[j]) for j in range(slots)]      # P_0 .. P_{K-1}, then hs^s_i
            powers.append(hs_chain(i))
            # the folds: block q multiplies the running product (P_0, then block q - 1's remainder) by P_{q+1}, the last one by hss
            table = S.mul_blocks([-1] + list(range(slots - 1)), [-(q + 2) for q in range(slots)], powers)
            roots.append(table[slots - 1])
        n_steps[0], n_steps[1] = 2 * m_bits, 2 * s_limbs * limb_bits
    # ---- suffix: assign_integer(res), assert_equal_fresh (once per result)
    ws = S.open()
    res_all, eq_cells = [], []
    for c_limbs in roots:
        res_c = _assign(ws, L, limb_bits, lb)
        g0 = ws.putc(0)
        eq_cell = ws.putc(1)
        for cc, rc in zip(c_limbs, res_c):
            _is_equal(ws, cc, rc)
            g = ws.putc(0)
            ws.gate(g)
            ws.put(eq_cell); ws.put()
            eq_cell = ws.put()
        res_all += res_c
        eq_cells.append(eq_cell)
    S.flush(ws)
    if dev is None:
        src, lookup_src = np.concatenate(S.src), np.concatenate(S.lk)
    else:
        cat = lambda parts: torch.cat([p_ if isinstance(p_, torch.Tensor) else torch.as_tensor(p_, dtype=torch.int64).to(dev) for p_ in parts])
        src, lookup_src = cat(S.src), cat(S.lk)
    for eq_cell in eq_cells:
        src[eq_cell] = -(1 + S.cid(1))      # assert_equal_fresh's result is constrained to the constant 1 (bench.rs:74)
    if kind == "partial":
        exposed = list(n_c) + list(v_c) + res_all[:L]
        for j in range(count):
            exposed += list(ct_c[j]) + res_all[(j + 1) * L:(j + 2) * L]
    elif kind in ("mix", "smix"):
        exposed = list(n_c) + list(hs_c) + [c for ct in ct_c for c in ct] + res_all
    elif kind == "pballot":
        exposed = list(n_c) + list(hs_c) + [c for g in gs_c for c in g] + res_all + sums_c
    elif kind in ("ballot", "sballot"):
        exposed = list(n_c) + list(g_c) + list(hs_c) + res_all + ([sum_c] if sum_c is not None else [])
    elif kind in ("tally", "wtally"):
        exposed = list(n_c) + [c for ct in ct_c for c in ct] + list(wt_c) + list(res_c)
    else:
        mid = list(x_c) + list(y_c) if kind == "add" else list(x_c) if statement == "decrypt" else []
        exposed = list(n_c) + list(g_c) + mid + list(res_c)
    return StructureArrays(n_cells=S.off, src=src, gate_mask=np.concatenate(S.mask), lookup_src=lookup_src,
                           constants=S.constants, result_cell=eq_cell, n_steps_g=n_steps[0], n_steps_r=n_steps[1],
                           public_cells=np.asarray(exposed, dtype=np.int64))


def columns(sa: StructureArrays, k: int, lb: int, minimum_rows: int = layout.MINIMUM_ROWS_BENCH, blinding_factors: int = layout.BLINDING_FACTORS,
            device: Optional[str] = None, keep_on_device: bool = False, break_rows: Optional[int] = None, expose: bool = False):
    """stream structure -> (CircuitStructure for prover.keygen, starts).  The permutation covers [advice | lookup advice | constants];
    every equality class becomes one cycle of sigma (cells in increasing (column, row) order).
    expose: add the instance column as the permutation's LAST column (public inputs): row i of it joins the class
    of sa.public_cells[i] -- as the greatest cell of that class, since the column is the last one.
    minimum_rows: the argument of the tester's calculate_params (layout.RowBudget): it fixes the NUMBER of advice / lookup-advice columns
    (20 on the reference's bench path, /root/reference/src/bench.rs:161-171; 9 under MockProver, src/paillier.rs:167-171); columns are
    FILLED to 2^k - (blinding_factors + 3) rows (break_rows overrides), so with 20 the last configured column can stay empty -- it is a
    column of the circuit all the same (selector all zero, identity permutation, committed and opened).
    starts: n_adv + 1 break points -- what K4 takes (pz_circuit_expand_cols_dev); a configured column the cells do not reach starts and
    ends at the stream's end.
    keep_on_device: selectors / map_col / map_row stay tensors on `device` (uint8 / int32) for prover.keygen instead of travelling to the
    host and back (4 GB each way at config c2)."""
    import torch

    n = 1 << k
    rb = layout.row_budget(k, minimum_rows, blinding_factors, break_rows)
    max_rows = rb.max_rows
    assert max_rows <= n - (blinding_factors + 1)
    starts = layout.break_points(sa.gate_mask, max_rows).astype(np.int64)
    A_used = starts.shape[0] - 1
    NC, NL, NK = sa.n_cells, sa.lookup_src.shape[0], len(sa.constants)
    A = rb.columns_for(NC, filled=A_used)
    Lk = rb.columns_for(NL)
    NP = int(sa.public_cells.shape[0]) if expose else 0
    m = A + Lk + 1 + (1 if expose else 0)
    assert NK <= max_rows
    if NP > max_rows:
        raise ValueError(f"{NP} public values do not fit the instance column's {max_rows} usable rows")
    if device is None:
        device = "cuda" if (torch.cuda.is_available() and NC > (1 << 22)) else "cpu"
    dev = torch.device(device)
    T0 = NC + NL + NK + (A_used - 1)
    T = T0 + NP                                   # ... | the instance cells
    st = torch.from_numpy(starts).to(dev)
    # ---- node -> flat position (column * n + row)
    pos = torch.empty(T, dtype=torch.int64, device=dev)
    c = torch.arange(NC, dtype=torch.int64, device=dev)
    col = torch.searchsorted(st, c, right=True) - 1
    col.clamp_(max=A_used - 1)
    pos[:NC] = col * n + (c - st[col])
    del c, col
    t = torch.arange(NL, dtype=torch.int64, device=dev)
    pos[NC:NC + NL] = (A + t // max_rows) * n + t % max_rows
    del t
    pos[NC + NL:NC + NL + NK] = (A + Lk) * n + torch.arange(NK, dtype=torch.int64, device=dev)
    j = torch.arange(1, A_used, dtype=torch.int64, device=dev)
    pos[NC + NL + NK:T0] = (j - 1) * n + (st[j] - st[j - 1])
    if NP:
        pos[T0:] = (A + Lk + 1) * n + torch.arange(NP, dtype=torch.int64, device=dev)
    # ---- what every node copies
    src = torch.arange(T, dtype=torch.int64, device=dev)
    s_adv = torch.as_tensor(sa.src).to(dev)
    src[:NC] = torch.where(s_adv < 0, NC + NL - 1 - s_adv, s_adv)          # -(1 + id) -> constant node NC + NL + id
    del s_adv
    src[NC:NC + NL] = torch.as_tensor(sa.lookup_src).to(dev)
    src[NC + NL + NK:T0] = st[j]
    del j
    if NP:
        src[T0:] = torch.from_numpy(np.ascontiguousarray(sa.public_cells, dtype=np.int64)).to(dev)
    while True:                                                           # roots by pointer jumping (chains are a few links long)
        nxt = src[src]
        if torch.equal(nxt, src):
            break
        src = nxt
    del nxt
    # ---- cycles: nodes sorted by (root, position); each maps to its successor, the last of a class to the first
    key_root = src
    touched = torch.zeros(T, dtype=torch.bool, device=dev)
    ids = torch.arange(T, dtype=torch.int64, device=dev)
    nonroot = key_root != ids
    touched[nonroot] = True
    touched[key_root[nonroot]] = True
    del nonroot
    members = ids[touched]
    del ids, touched
    r_m, p_m = key_root[members], pos[members]
    del key_root
    # sorted by (class, position): one sort of the combined key (class < T < 2^31, position < m n < 2^31 at every supported size)
    span = m * n
    assert T < (1 << 31) and span < (1 << 31)
    key, _ = torch.sort(r_m * span + p_m)
    r_m, p_m = key // span, key % span
    del key, members
    first = torch.ones_like(r_m, dtype=torch.bool)
    first[1:] = r_m[1:] != r_m[:-1]
    firsts = torch.nonzero(first).view(-1)                 # index of every class's first member ...
    start_of = firsts[torch.cumsum(first.to(torch.int64), 0) - 1]   # ... broadcast over its members (a cumsum, not torch.cummax: that
    #                                                                   scan-with-indices kernel took 0.9 s on 2 x 10^8 elements)
    nxt_p = torch.empty_like(p_m)
    nxt_p[:-1] = p_m[1:]
    last = torch.ones_like(first)
    last[:-1] = first[1:]
    nxt_p[last] = p_m[start_of[last]]
    image = torch.arange(m * n, dtype=torch.int64, device=dev)
    image[p_m] = nxt_p
    map_col, map_row = (image // n).to(torch.int32).view(m, n), (image % n).to(torch.int32).view(m, n)
    del image, p_m, nxt_p, r_m
    # ---- selectors: the gate of a shared break cell is enabled in the column it starts
    gi = torch.nonzero(torch.from_numpy(sa.gate_mask).to(dev)).view(-1)
    sel = torch.zeros(A * n, dtype=torch.uint8, device=dev)
    sel[pos[gi]] = 1
    selectors = sel.view(A, n)
    if not keep_on_device:
        map_col = map_col.cpu().numpy().view(np.uint32)
        map_row = map_row.cpu().numpy().view(np.uint32)
        selectors = selectors.cpu().numpy()
    public = None
    if expose:
        pc = pos[torch.from_numpy(np.ascontiguousarray(sa.public_cells, dtype=np.int64)).to(dev)].cpu().numpy()
        public = [(int(p_) // n, int(p_) % n) for p_ in pc]
    cs = CircuitStructure(k=k, lookup_bits=lb, max_rows=max_rows, blinding_factors=blinding_factors, selectors=selectors, n_lk=Lk,
                          constants=list(sa.constants), map_col=map_col, map_row=map_row, minimum_rows=minimum_rows, n_adv_used=A_used,
                          n_instance=1 if expose else 0, public_cells=public)
    starts = np.concatenate([starts, np.full(A - A_used, NC, dtype=np.int64)])
    return cs, starts.astype(np.uint64)
