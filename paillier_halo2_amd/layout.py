"""Shape arithmetic of the Paillier-encrypt circuit: how many advice / lookup cells the
BigUintChip operations behind PaillierChip::encrypt (paillier.rs:32-60) push into halo2-lib's
Context, hence how many 2^k-row columns, MSMs and NTTs one proof needs.

The cell-emitting code lives in un-vendored dependencies (biguint-halo2, halo2-base, halo2-ecc:
Cargo.toml:9-11, no rev) -- SURVEY.md tags it [D].  The counts below restate the halo2-rsa
BigUintChip lineage on halo2-lib v0.4 gate primitives and are the SPEC the K4 expansion kernel
(csrc/pz_witness.hip) implements; DESIGN.md section 4 lists the per-primitive cell patterns.  Layout parity
with the reference's dependency versions is unpinned (they float); the VALUES in the cells are
determined by the step trace.
"""
from __future__ import annotations

import math
from dataclasses import dataclass


# ---- the row budget of a column (halo2-lib's tester, reached from /root/reference/src/bench.rs:161-171 and src/paillier.rs:167-171) [D]
BLINDING_FACTORS = 6          # cs.blinding_factors() of halo2-lib's circuits: max(3, the basic gate's 4 rotations) + 2
MINIMUM_ROWS_BENCH = 20       # bench_builder: builder.calculate_params(Some(20))   
MINIMUM_ROWS_MOCK = 9         # base_test().run(..): builder.calculate_params(Some(9)) before MockProver::run


@dataclass(frozen=True)
class RowBudget:
    """Two different row counts shape a halo2-lib circuit, and the reference's two test paths differ in the first:
    count_rows = 2^k - minimum_rows   what calculate_params(Some(minimum_rows)) divides the cell totals by: the NUMBER of advice /
                                      lookup-advice columns the circuit is configured with (20 on the bench path, 9 under MockProver);
    max_rows   = 2^k - unusable_rows  how far a column is FILLED: FlexGateConfig::max_rows = 2^k - cs.minimum_rows(), and
                                      cs.minimum_rows() = blinding_factors + 3 = 9 -- what assign_with_constraints breaks columns at.
    With minimum_rows = 20 the configured column count can exceed the columns the cells fill (the last one stays empty: it is still
    committed, opened and part of the permutation).  Both numbers restate dependency behaviour (halo2-lib v0.4 lineage, SURVEY tag
    [D]: unpinned); `break_rows` overrides max_rows for a dependency version that fills columns to 2^k - minimum_rows instead."""
    k: int
    minimum_rows: int
    unusable_rows: int

    @property
    def n(self) -> int:
        return 1 << self.k

    @property
    def count_rows(self) -> int:
        return self.n - self.minimum_rows

    @property
    def max_rows(self) -> int:
        return self.n - self.unusable_rows

    def columns_for(self, cells: int, filled: int | None = None) -> int:
        """configured columns for a stream of `cells` cells of which the fill needs `filled` (default: a plain cut at max_rows)"""
        used = -(-cells // self.max_rows) if filled is None else filled
        return max(used, -(-cells // self.count_rows))


def row_budget(k: int, minimum_rows: int = MINIMUM_ROWS_BENCH, blinding_factors: int = BLINDING_FACTORS, break_rows: int | None = None) -> RowBudget:
    unusable = blinding_factors + 3 if break_rows is None else (1 << k) - break_rows
    assert unusable >= blinding_factors + 1 and minimum_rows >= 0
    return RowBudget(k, minimum_rows, unusable)


def range_check_cells(bits: int, lookup_bits: int):
    """halo2-lib RangeChip::range_check(a, bits): (advice cells, lookup cells)."""
    k = -(-bits // lookup_bits)
    rem = bits % lookup_bits
    adv = 0 if k == 1 else 1 + 3 * (k - 1)
    lk = k
    if rem == 1:
        adv += 4  # assert_bit gate
    elif rem > 1:
        adv += 4  # gate.mul(last_limb, 2^(lookup_bits-rem))
        lk += 1
    return adv, lk


def mul_word_max_bits(limb_bits: int, min_n: int) -> int:
    """bits_size(2 * (min_n*(2^limb_bits-1)^2 + (2^limb_bits-1)))  (is_equal_muled's carry bound)"""
    m = (1 << limb_bits) - 1
    return (2 * (min_n * m * m + m)).bit_length()


@dataclass
class StepCells:
    advice: int
    lookup: int
    # offsets of the segments inside one step's advice block (the K4 kernel's layout)
    seg: dict


def mul_mod_cells(limbs: int, limb_bits: int, lookup_bits: int) -> StepCells:
    """Cells one BigUintChip::mul_mod(a, b, n) emits, all operands `limbs` limbs."""
    L = limbs
    D = 2 * L - 1  # limbs of a product
    seg = {}
    off = 0
    rc_adv, rc_lk = range_check_cells(limb_bits, lookup_bits)
    # 1. assign_integer(q), assign_integer(n), assign_integer(r): L witness cells + L range checks each
    seg["assign"] = off
    off += 3 * (L + L * rc_adv)
    lookups = 3 * L * rc_lk
    # 2. mul(a, b) and mul(q, n): load_zero + truncated mul_no_carry over D limbs
    per_mul = 1 + sum(1 + 3 * (i + 1) for i in range(D))
    seg["mul_ab"] = off
    off += per_mul
    seg["mul_qn"] = off
    off += per_mul
    # 3. qn + r: L gate.add
    seg["add_r"] = off
    off += 4 * L
    # 4. is_equal_muled over D limbs
    cb = mul_word_max_bits(limb_bits, L) - limb_bits
    cb_adv, cb_lk = range_check_cells(cb, lookup_bits)
    per_limb = 4 + 7 + 22 + 4 + 22 + 12 + 4  # sub, sum3, div_mod, add, div_mod, is_equal, and
    seg["eq"] = off
    off += 2 + D * per_limb + (D - 1) * cb_adv + (12 + 4)  # load_zero/one + limbs + carry checks + final carry
    lookups += (D - 1) * cb_lk
    # 5. r < n : big_less_than over L limbs (sub with borrow, one range check per limb)
    lt_adv, lt_lk = range_check_cells(limb_bits, lookup_bits)
    seg["lt"] = off
    off += L * (11 + lt_adv) + 1
    lookups += L * lt_lk
    seg["end"] = off
    return StepCells(off, lookups, seg)


def refresh_aux(limb_bits: int, num_limbs_l: int, num_limbs_r: int):
    """RefreshAux::new(limb_bits, l, r).increased_limbs_vec (paillier.rs:40-44): how many further limbs the maximal
    value of each product limb spills into when it is cut back to limb_bits-wide limbs; its length is the limb count
    of the refreshed integer (l + r for the shapes of this circuit)."""
    mx = (1 << limb_bits) - 1
    d = num_limbs_l + num_limbs_r - 1
    muled = [sum(1 for j in range(num_limbs_l) if 0 <= i - j < num_limbs_r) * mx * mx for i in range(d)]
    inc = []
    cur = 0
    while cur < len(muled):
        chunks = max(1, -(-muled[cur].bit_length() // limb_bits))
        inc.append(chunks - 1)
        val = muled[cur]
        for i in range(chunks):
            piece, val = val & mx, val >> limb_bits
            if cur + i < len(muled):
                muled[cur + i] = piece if i == 0 else muled[cur + i] + piece
            else:
                muled.append(piece)
        cur += 1
    return inc


def assign_cells(num_limbs: int, limb_bits: int, lookup_bits: int):
    """assign_integer: the limbs as witnesses, then one range check each -> (advice, lookup)"""
    a, l = range_check_cells(limb_bits, lookup_bits)
    return num_limbs * (1 + a), num_limbs * l


def square_cells(limbs: int) -> int:
    """square(n) = mul(n, n): load_zero + truncated mul_no_carry over 2 limbs - 1 product limbs"""
    return 1 + sum(1 + 3 * (i + 1) for i in range(2 * limbs - 1))


def refresh_cells(inc, limb_bits: int, lookup_bits: int):
    a, l = range_check_cells(limb_bits, lookup_bits)
    adv = 1 + sum((k + 1) * 22 + k * 4 for k in inc) + len(inc) * a
    return adv, len(inc) * l


def assert_equal_cells(limbs: int) -> int:
    return 2 + 16 * limbs


@dataclass
class CircuitCells:
    advice: int
    lookup: int
    seg: dict   # name -> (advice offset, lookup offset), in emission order


TALLY_MAX = 65536     # ciphertexts of one tally (pz.h pz_paillier_tally)


def tally_tree(count: int):
    """The product tree of a tally: level by level the neighbours of the current list are multiplied, an odd
    last element is carried up without a product.  -> [(a, b)] per mul_mod block in level-major order; an operand >= 0 is the
    block that produced it, -(1 + i) the ciphertext c_(i+1)."""
    if not 2 <= count <= TALLY_MAX:
        raise ValueError(f"a tally takes 2 .. {TALLY_MAX} ciphertexts, not {count}")
    cur = [-(1 + i) for i in range(count)]
    blocks = []
    while len(cur) > 1:
        nxt = []
        for j in range(len(cur) // 2):
            nxt.append(len(blocks))
            blocks.append((cur[2 * j], cur[2 * j + 1]))
        if len(cur) & 1:
            nxt.append(cur[-1])
        cur = nxt
    return blocks


WTALLY_MAX_BITS = 64  # width of a weight of the weighted tally (pz.h pz_paillier_wtally): one 64-bit word


def wtally_tree(count: int):
    """tally_tree over the B powers c_i^w_i of a weighted tally; B = 1 has no tree (the root is the power itself)"""
    if not 1 <= count <= TALLY_MAX:
        raise ValueError(f"a weighted tally takes 1 .. {TALLY_MAX} ciphertexts, not {count}")
    return tally_tree(count) if count > 1 else []


BALLOT_MAX = 1024       # ciphertexts of one ballot (pz.h pz_paillier_ballot)
BALLOT_MAX_BITS = 64    # width of a ballot entry's message: one 64-bit word
PARTIAL_MAX = 1024      # ciphertexts one trustee opens in one proof (pz.h pz_paillier_partial)
MIX_MAX = 1024          # ciphertexts of one mix, a power of two (pz.h pz_paillier_mix)
PBALLOT_MAX_SLOTS = 64  # slots of one packed ballot (pz.h pz_paillier_pballot); count * slots <= BALLOT_MAX


def circuit_cells(kind: str, limbs_n: int, limb_bits: int, lookup_bits: int, n_steps_g: int = 0, n_steps_r: int = 0,
                  count: int | None = None, w_bits: int | None = None, m_bits: int | None = None,
                  s_limbs: int | None = None, slots: int | None = None) -> CircuitCells:
    """The whole cell stream of paillier_enc_test (bench.rs:33-75, kind 'encrypt') or paillier_enc_add_test
    (bench.rs:77-117, kind 'add'), operation by operation in call order -- what pz_circuit_expand_dev writes.
    kind 'tally' (count = B ciphertexts): assign n, assign c_1 .. c_B at full width, square + refresh once, the B - 1 blocks of
    tally_tree, assign res, assert_equal_fresh -- no load_zero, no g, no pow_mod constants.
    kind 'wtally' (count = B ciphertexts, w_bits = W bits per weight): assign n, assign c_1 .. c_B at full
    width, load_witness(w_1 .. w_B), square + refresh once, per ciphertext pow_mod(c_i, w_i) over W in-circuit bits ([1, 0],
    num_to_bits, W blocks of mul_mod + select + square_mod), the B - 1 blocks of the tree over the powers, assign res,
    assert_equal_fresh.
    kind 'decrypt' (circuit kind 5): 'encrypt_uniform' cell for cell -- its statement alone differs.
    kind 'ballot' (circuit kind 6; count = K ciphertexts, m_bits = b bits per message, n_steps_r = the records
    of ONE r^n chain): assign n, g, load_witness(m_1 .. m_K), for K >= 2 FlexGate::sum of them (1 + 3 (K - 1) cells), assign r_1 .. r_K,
    square + refresh once, load_zero, per ciphertext pow_mod(g, m_i) over b in-circuit bits, pow_mod_fixed_exp(r_i, n) and the final
    mul_mod, then per ciphertext assign res_i and assert_equal_fresh.
    kind 'partial' (circuit kind 7; count = K ciphertexts one trustee opens): assign n, assign v, theta and
    c_1 .. c_K at full width, square + refresh once, load_zero, pow_mod(v, theta) over all 2 Ln limbs of theta as kind 2 emits pow_mod,
    per ciphertext mul_mod(c_j, c_j) and pow_mod(s_j, theta), then assign + assert_equal_fresh for h and every u_j.
    kind 'mix' (circuit kind 8; count = K = 2^d ciphertexts, n_steps_r = the records of ONE r^n chain): assign
    n, assign c_1 .. c_K at full width, assign r_1 .. r_K, square + refresh once, load_zero, the (2d - 1) K / 2 switches of the network
    (assert_bit's 4 cells, then per limb two selects of 8 cells), per output [1, 0], the r^n chain's blocks and the final mul_mod, then
    per output assign res_i and assert_equal_fresh.
    kind 'sballot' (circuit kind 9; count = K ciphertexts, m_bits = b bits per message, s_limbs limbs per
    exponent s_i): assign n, g, assign hs at full width, load_witness(m_1 .. m_K), for K >= 2 FlexGate::sum of them, assign s_1 .. s_K
    (s_limbs limbs each), square + refresh once, load_zero, per ciphertext pow_mod(g, m_i) over b in-circuit bits as 'ballot',
    pow_mod(hs, s_i) as 'partial' emits a chain over the s_limbs limbs of s_i, and the final mul_mod, then per ciphertext assign res_i
    and assert_equal_fresh.  No step count enters: nothing of the key but its size shapes the stream.
    kind 'smix' (circuit kind 10; count = K = 2^d ciphertexts, s_limbs limbs per exponent s_i): assign n, assign
    hs and c_1 .. c_K at full width, assign s_1 .. s_K (s_limbs limbs each), square + refresh once, load_zero, the network as 'mix', per
    output [1, 0], pow_mod(hs, s_i) as 'sballot' emits its hs-chain and the final mul_mod(d_i, hss_i), then per output assign res_i and
    assert_equal_fresh.  No step count enters: the shape is (K, s_limbs) and the key size.
    kind 'pballot' (circuit kind 11; count = R ciphertexts, slots = K values of m_bits = b bits in each, s_limbs
    limbs per exponent s_i): assign n, assign hs and the K slot bases G_j at full width, load_witness of the R K values, for K >= 2 one
    FlexGate::sum per ciphertext, assign s_1 .. s_R (s_limbs limbs each), square + refresh once, load_zero, per ciphertext the K slot
    chains ([1, 0], num_to_bits, b bit blocks each, as 'ballot's g-chain), pow_mod(hs, s_i) as 'sballot' and the K fold blocks, then
    per ciphertext assign res_i and assert_equal_fresh.  The shape is (R, K, b, s_limbs) and the key size."""
    Ln, L = limbs_n, 2 * limbs_n
    if kind == "decrypt":
        kind = "encrypt_uniform"
    if kind == "tally":
        if count is None or not 2 <= count <= TALLY_MAX:
            raise ValueError(f"a tally takes count = 2 .. {TALLY_MAX} ciphertexts, not {count}")
        if n_steps_g not in (0, count - 1) or n_steps_r:
            raise ValueError("a tally of count ciphertexts has count - 1 steps")
    elif kind == "wtally":
        if count is None or not 1 <= count <= TALLY_MAX:
            raise ValueError(f"a weighted tally takes count = 1 .. {TALLY_MAX} ciphertexts, not {count}")
        if w_bits is None or not 1 <= w_bits <= WTALLY_MAX_BITS:
            raise ValueError(f"a weight has w_bits = 1 .. {WTALLY_MAX_BITS} bits, not {w_bits}")
        if n_steps_g not in (0, 2 * count * w_bits) or n_steps_r not in (0, count - 1):
            raise ValueError("a weighted tally has 2 * count * w_bits chain steps and count - 1 tree steps")
    elif kind == "ballot":
        if count is None or not 1 <= count <= BALLOT_MAX:
            raise ValueError(f"a ballot takes count = 1 .. {BALLOT_MAX} ciphertexts, not {count}")
        if m_bits is None or not 1 <= m_bits <= BALLOT_MAX_BITS:
            raise ValueError(f"a ballot's message has m_bits = 1 .. {BALLOT_MAX_BITS} bits, not {m_bits}")
        if n_steps_g not in (0, 2 * m_bits) or n_steps_r < 1:
            raise ValueError("a ballot entry has 2 * m_bits g-chain steps and n_steps_r >= 1 steps of one r^n chain")
    elif kind == "partial":
        if count is None or not 1 <= count <= PARTIAL_MAX:
            raise ValueError(f"a trustee opens count = 1 .. {PARTIAL_MAX} ciphertexts in one proof, not {count}")
        if n_steps_g not in (0, 2 * L * limb_bits) or n_steps_r:
            raise ValueError("a partial decryption's chain has 2 * (2 * limbs_n * limb_bits) steps")
    elif kind == "mix":
        if count is None or not (1 <= count <= MIX_MAX and count & (count - 1) == 0):
            raise ValueError(f"a mix takes count = 1, 2, 4 .. {MIX_MAX} ciphertexts, not {count}")
        if n_steps_g or n_steps_r < 1:
            raise ValueError("a mix has no g-chain and n_steps_r >= 1 steps of one r^n chain")
    elif kind == "sballot":
        if count is None or not 1 <= count <= BALLOT_MAX:
            raise ValueError(f"a ballot takes count = 1 .. {BALLOT_MAX} ciphertexts, not {count}")
        if m_bits is None or not 1 <= m_bits <= BALLOT_MAX_BITS:
            raise ValueError(f"a ballot's message has m_bits = 1 .. {BALLOT_MAX_BITS} bits, not {m_bits}")
        if s_limbs is None or not 1 <= s_limbs <= L:
            raise ValueError(f"a short-randomness ballot's exponent has s_limbs = 1 .. {L} limbs, not {s_limbs}")
        if n_steps_g not in (0, 2 * m_bits) or n_steps_r not in (0, 2 * s_limbs * limb_bits):
            raise ValueError("a short-randomness ballot entry has 2 * m_bits g-chain steps and 2 * s_limbs * limb_bits hs-chain steps")
    elif kind == "smix":
        if count is None or not (1 <= count <= MIX_MAX and count & (count - 1) == 0):
            raise ValueError(f"a mix takes count = 1, 2, 4 .. {MIX_MAX} ciphertexts, not {count}")
        if s_limbs is None or not 1 <= s_limbs <= L:
            raise ValueError(f"a short-randomness mix's exponent has s_limbs = 1 .. {L} limbs, not {s_limbs}")
        if n_steps_g or n_steps_r not in (0, 2 * s_limbs * limb_bits):
            raise ValueError("a short-randomness mix has no g-chain and 2 * s_limbs * limb_bits steps of one hs-chain")
    elif kind == "pballot":
        if count is None or not 1 <= count <= BALLOT_MAX:
            raise ValueError(f"a packed ballot takes count = 1 .. {BALLOT_MAX} ciphertexts, not {count}")
        if slots is None or not 1 <= slots <= PBALLOT_MAX_SLOTS or count * slots > BALLOT_MAX:
            raise ValueError(f"a packed ballot has slots = 1 .. {PBALLOT_MAX_SLOTS} with count * slots <= {BALLOT_MAX}, not {slots}")
        if m_bits is None or not 1 <= m_bits <= BALLOT_MAX_BITS:
            raise ValueError(f"a slot value has m_bits = 1 .. {BALLOT_MAX_BITS} bits, not {m_bits}")
        if s_limbs is None or not 1 <= s_limbs <= L:
            raise ValueError(f"a packed ballot's exponent has s_limbs = 1 .. {L} limbs, not {s_limbs}")
        if n_steps_g not in (0, 2 * m_bits) or n_steps_r not in (0, 2 * s_limbs * limb_bits):
            raise ValueError("a packed ballot has 2 * m_bits steps per slot chain and 2 * s_limbs * limb_bits hs-chain steps")
    elif count is not None:
        raise ValueError("count belongs to kinds 'tally', 'wtally', 'ballot', 'partial', 'mix', 'sballot', 'smix' and 'pballot'")
    if w_bits is not None and kind != "wtally":
        raise ValueError("w_bits belongs to kind 'wtally'")
    if m_bits is not None and kind not in ("ballot", "sballot", "pballot"):
        raise ValueError("m_bits belongs to kinds 'ballot', 'sballot' and 'pballot'")
    if s_limbs is not None and kind not in ("sballot", "smix", "pballot"):
        raise ValueError("s_limbs belongs to kinds 'sballot', 'smix' and 'pballot'")
    if slots is not None and kind != "pballot":
        raise ValueError("slots belongs to kind 'pballot'")
    mm = mul_mod_cells(L, limb_bits, lookup_bits)
    seg, a, l = {}, 0, 0

    def put(name, da, dl=0):
        nonlocal a, l
        seg[name] = (a, l)
        a += da
        l += dl

    if kind == "partial":
        put("assign_n", *assign_cells(Ln, limb_bits, lookup_bits))
        ca, cl = assign_cells(L, limb_bits, lookup_bits)
        put("assign_v", ca, cl)
        put("assign_theta", ca, cl)
        put("assign_cts", count * ca, count * cl)
    elif kind == "mix":
        na, nl = assign_cells(Ln, limb_bits, lookup_bits)
        ca, cl = assign_cells(L, limb_bits, lookup_bits)
        put("assign_n", na, nl)
        put("assign_cts", count * ca, count * cl)
        put("assign_rs", count * na, count * nl)
    elif kind == "smix":
        ca, cl = assign_cells(L, limb_bits, lookup_bits)
        put("assign_n", *assign_cells(Ln, limb_bits, lookup_bits))
        put("assign_hs", ca, cl)
        put("assign_cts", count * ca, count * cl)
        sa, sl = assign_cells(s_limbs, limb_bits, lookup_bits)
        put("assign_ss", count * sa, count * sl)
    elif kind == "ballot":
        na, nl = assign_cells(Ln, limb_bits, lookup_bits)
        put("assign_n", na, nl)
        put("assign_g", na, nl)
        put("messages", count)
        if count >= 2:
            put("sum", 1 + 3 * (count - 1))
        put("assign_rs", count * na, count * nl)
    elif kind == "sballot":
        na, nl = assign_cells(Ln, limb_bits, lookup_bits)
        put("assign_n", na, nl)
        put("assign_g", na, nl)
        put("assign_hs", *assign_cells(L, limb_bits, lookup_bits))
        put("messages", count)
        if count >= 2:
            put("sum", 1 + 3 * (count - 1))
        sa, sl = assign_cells(s_limbs, limb_bits, lookup_bits)
        put("assign_ss", count * sa, count * sl)
    elif kind == "pballot":
        ca, cl = assign_cells(L, limb_bits, lookup_bits)
        put("assign_n", *assign_cells(Ln, limb_bits, lookup_bits))
        put("assign_hs", ca, cl)
        put("assign_bases", slots * ca, slots * cl)
        put("values", count * slots)
        if slots >= 2:
            put("sums", count * (1 + 3 * (slots - 1)))
        sa, sl = assign_cells(s_limbs, limb_bits, lookup_bits)
        put("assign_ss", count * sa, count * sl)
    elif kind in ("tally", "wtally"):
        put("assign_n", *assign_cells(Ln, limb_bits, lookup_bits))
        ca, cl = assign_cells(L, limb_bits, lookup_bits)
        put("assign_cts", count * ca, count * cl)
        if kind == "wtally":
            put("weights", count)
    else:
        for name in ("assign_n", "assign_g", "assign_x", "assign_y"):
            put(name, *assign_cells(Ln, limb_bits, lookup_bits))
    put("square", square_cells(Ln))
    put("refresh", *refresh_cells(refresh_aux(limb_bits, Ln, Ln), limb_bits, lookup_bits))
    if kind == "tally":
        put("tree", (count - 1) * mm.advice, (count - 1) * mm.lookup)
    elif kind == "wtally":
        # per chain: assign_constant(1), load_zero, num_to_bits (7 W - 2 cells), W blocks of mul_mod + select + square_mod
        put("chains", count * (2 + 7 * w_bits - 2 + w_bits * (2 * mm.advice + 8 * L)), count * 2 * w_bits * mm.lookup)
        put("tree", (count - 1) * mm.advice, (count - 1) * mm.lookup)
    else:
        put("load_zero", 1)
    if kind == "encrypt":
        put("pow_g", 2 + n_steps_g * mm.advice, n_steps_g * mm.lookup)
        put("pow_r", 2 + n_steps_r * mm.advice, n_steps_r * mm.lookup)
    elif kind == "encrypt_uniform":
        # g^m as pow_mod over Ln * limb_bits in-circuit bits: per limb of m num_to_bits (7 W - 2 cells), per
        # bit two mul_mods and a limb-wise select (8 cells per limb); the step count is fixed by the key size
        m_bits = Ln * limb_bits
        assert n_steps_g in (0, 2 * m_bits)
        put("pow_g", 2 + Ln * (7 * limb_bits - 2) + m_bits * (2 * mm.advice + 8 * L), 2 * m_bits * mm.lookup)
        put("pow_r", 2 + n_steps_r * mm.advice, n_steps_r * mm.lookup)
    if kind == "ballot":
        # per entry: [1, 0], num_to_bits (7 b - 2 cells), b blocks of mul_mod + select + square_mod; [1, 0] and the r^n chain's blocks;
        # the final block.  Then per entry assign res_i at full width and assert_equal_fresh
        steps = 2 * m_bits + n_steps_r + 1
        put("entries", count * (2 + 7 * m_bits - 2 + m_bits * 8 * L + 2 + steps * mm.advice), count * steps * mm.lookup)
        ra, rl = assign_cells(L, limb_bits, lookup_bits)
        put("results", count * (ra + assert_equal_cells(L)), count * rl)
        seg["end"] = (a, l)
        return CircuitCells(a, l, seg)
    if kind == "sballot":
        # per entry: the g-chain as 'ballot'; [1, 0], then per limb of s_i num_to_bits (7 W - 2 cells) and W blocks of mul_mod + select
        # + square_mod; the final block.  Then per entry assign res_i at full width and assert_equal_fresh
        s_bits = s_limbs * limb_bits
        steps = 2 * m_bits + 2 * s_bits + 1
        put("entries", count * (2 + 7 * m_bits - 2 + 2 + s_limbs * (7 * limb_bits - 2) + (m_bits + s_bits) * 8 * L + steps * mm.advice),
            count * steps * mm.lookup)
        ra, rl = assign_cells(L, limb_bits, lookup_bits)
        put("results", count * (ra + assert_equal_cells(L)), count * rl)
        seg["end"] = (a, l)
        return CircuitCells(a, l, seg)
    if kind == "pballot":
        # per ciphertext: K slot chains ([1, 0], num_to_bits of 7 b - 2 cells, b blocks of mul_mod + select + square_mod); [1, 0], then per
        # limb of s_i num_to_bits (7 W - 2 cells) and W such blocks; the K fold blocks.  Then per ciphertext assign res_i and
        # assert_equal_fresh
        s_bits = s_limbs * limb_bits
        steps = 2 * m_bits * slots + 2 * s_bits + slots
        put("entries", count * (slots * (2 + 7 * m_bits - 2) + 2 + s_limbs * (7 * limb_bits - 2) + (slots * m_bits + s_bits) * 8 * L
                                + steps * mm.advice), count * steps * mm.lookup)
        ra, rl = assign_cells(L, limb_bits, lookup_bits)
        put("results", count * (ra + assert_equal_cells(L)), count * rl)
        seg["end"] = (a, l)
        return CircuitCells(a, l, seg)
    if kind == "mix":
        # per switch assert_bit (4 cells) and per limb two selects (8 cells each); per output [1, 0], the chain's blocks and the final
        # block; then per output assign res_i at full width and assert_equal_fresh
        layers = 2 * (count.bit_length() - 1) - 1 if count > 1 else 0
        put("network", layers * (count // 2) * (4 + 16 * L))
        put("outputs", count * (2 + (n_steps_r + 1) * mm.advice), count * (n_steps_r + 1) * mm.lookup)
        ra, rl = assign_cells(L, limb_bits, lookup_bits)
        put("results", count * (ra + assert_equal_cells(L)), count * rl)
        seg["end"] = (a, l)
        return CircuitCells(a, l, seg)
    if kind == "smix":
        # the network as 'mix'; per output [1, 0], then per limb of s_i num_to_bits (7 W - 2 cells) and W blocks of mul_mod + select +
        # square_mod, and the final block; then per output assign res_i at full width and assert_equal_fresh
        layers = 2 * (count.bit_length() - 1) - 1 if count > 1 else 0
        put("network", layers * (count // 2) * (4 + 16 * L))
        s_bits = s_limbs * limb_bits
        steps = 2 * s_bits + 1
        put("outputs", count * (2 + s_limbs * (7 * limb_bits - 2) + s_bits * 8 * L + steps * mm.advice), count * steps * mm.lookup)
        ra, rl = assign_cells(L, limb_bits, lookup_bits)
        put("results", count * (ra + assert_equal_cells(L)), count * rl)
        seg["end"] = (a, l)
        return CircuitCells(a, l, seg)
    if kind == "partial":
        # per chain: [1, 0], then per limb of theta num_to_bits (7 W - 2 cells) and W blocks of mul_mod + select + square_mod; a
        # squaring block in front of every chain but the first.  Then assign + assert_equal_fresh for h and every u_j
        e_bits = L * limb_bits
        chain = 2 + L * (7 * limb_bits - 2) + e_bits * (2 * mm.advice + 8 * L)
        put("chains", (count + 1) * chain + count * mm.advice, (count + (count + 1) * 2 * e_bits) * mm.lookup)
        ra, rl = assign_cells(L, limb_bits, lookup_bits)
        put("results", (count + 1) * (ra + assert_equal_cells(L)), (count + 1) * rl)
        seg["end"] = (a, l)
        return CircuitCells(a, l, seg)
    if kind not in ("tally", "wtally"):
        put("final", mm.advice, mm.lookup)
    put("assign_res", *assign_cells(L, limb_bits, lookup_bits))
    put("assert_equal", assert_equal_cells(L))
    seg["end"] = (a, l)
    return CircuitCells(a, l, seg)


@dataclass
class ProofShape:
    k: int
    lookup_bits: int
    limbs: int
    n_steps: int
    cells_per_step: int
    lookups_per_step: int
    advice_cols: int
    lookup_cols: int
    perm_cols: int
    msm_witness: int      # commit_lagrange of advice columns (short scalars)
    msm_lookup: int       # commit_lagrange of lookup-advice columns (lookup_bits-bit scalars)
    msm_full: int         # permuted lookup columns, lookup/permutation products, h pieces, openings
    polys: int            # polynomials taken Lagrange -> coeff -> extended coset
    ext_k: int
    advice_cells: int = 0   # the whole circuit's stream (circuit_cells)
    lookup_cells: int = 0


def encrypt_proof_shape(enc_bits: int, k: int, n_steps: int, limb_bits: int = 64, lookup_bits: int | None = None,
                        minimum_rows: int = MINIMUM_ROWS_BENCH, max_degree: int = 4, kind: str = "encrypt", n_steps_g: int | None = None,
                        blinding_factors: int = BLINDING_FACTORS) -> ProofShape:
    """Column / MSM / NTT counts of one encrypt (or add) proof (SURVEY.md section 3.4's table, made concrete).  n_steps
    counts every mul_mod of the circuit (both chains + the final one); the split between the chains only moves the four
    constant cells of pow_mod_fixed_exp and does not change any count."""
    if lookup_bits is None:
        lookup_bits = k - 1  # the reference's pattern: paillier.rs:168-169, bench.rs:162-163
    Ln = enc_bits // limb_bits
    L = 2 * Ln
    sc = mul_mod_cells(L, limb_bits, lookup_bits)
    rb = row_budget(k, minimum_rows, blinding_factors)
    if kind == "encrypt":
        ng = (n_steps - 1) // 2 if n_steps_g is None else n_steps_g
        cc = circuit_cells("encrypt", Ln, limb_bits, lookup_bits, ng, n_steps - 1 - ng)
    elif kind == "encrypt_uniform":   # g^m takes 2 * (Ln * limb_bits) steps whatever the message is
        ng = 2 * Ln * limb_bits
        cc = circuit_cells("encrypt_uniform", Ln, limb_bits, lookup_bits, ng, n_steps - 1 - ng)
    else:
        cc = circuit_cells("add", Ln, limb_bits, lookup_bits)
    A = rb.columns_for(cc.advice)     # (plain cut; the break-point layout of circuit_structure.columns loses 1-3 rows per column)
    Lk = rb.columns_for(cc.lookup)
    P = math.ceil((A + Lk + 1) / (max_degree - 2))
    return ProofShape(k=k, lookup_bits=lookup_bits, limbs=L, n_steps=n_steps, cells_per_step=sc.advice,
                      lookups_per_step=sc.lookup, advice_cols=A, lookup_cols=Lk, perm_cols=P, msm_witness=A,
                      msm_lookup=Lk, msm_full=3 * Lk + P + 1 + (max_degree - 1) + 2, polys=A + 4 * Lk + P,
                      ext_k=k + 2, advice_cells=cc.advice, lookup_cells=cc.lookup)


def break_points(gate_mask, max_rows: int):
    """halo2-lib's break-point column layout of an advice stream (pz.h pz_circuit_break_points; host logic inside the C ABI library,
    no device needed): gate_mask = uint8 array, 1 where a gate window starts.  -> uint64 array of n_cols + 1 stream indices:
    column j holds the cells starts[j] .. starts[j + 1] from row 0 on (the cell it ends with is also row 0 of column j + 1)."""
    import ctypes as C

    import numpy as np

    from . import _lib

    m = np.ascontiguousarray(gate_mask, dtype=np.uint8)
    L = _lib.lib()
    nc = C.c_size_t()
    rc = L.pz_circuit_break_points(C.c_void_p(m.ctypes.data), m.shape[0], max_rows, None, 0, C.byref(nc))
    if rc != 0:
        raise _lib.PzError(rc, "pz_circuit_break_points")
    out = np.zeros(nc.value + 1, dtype=np.uint64)
    rc = L.pz_circuit_break_points(C.c_void_p(m.ctypes.data), m.shape[0], max_rows, C.c_void_p(out.ctypes.data), out.shape[0], C.byref(nc))
    if rc != 0:
        raise _lib.PzError(rc, "pz_circuit_break_points")
    return out
