"""TEST INFRASTRUCTURE: the reference for PUBLIC INPUTS (one instance column) in Python integers, on top of the
oracle (oracle/pyref.py, oracle/circuit.py, oracle/verifier.py, all unmodified): the exposed cells from the oracle's own walk of the
circuit WITH values, the copy constraints extended by (exposed cell i) == (instance column, row i), the instance column at a point,
the verifier's expected h(x) with the extra permuted value, the transcript replay that absorbs the statement first, and the query
layout with m + 1 sigma members.  Nothing here is shared with the product's code."""
from __future__ import annotations

import hashlib
import struct
from typing import Dict, List, Sequence

import numpy as np

from oracle import circuit as CQ
from oracle import pyref as P
from oracle import verifier as V

R = P.FR_R

# the three shapes of the feature's tests: kind, enc_bits, limb_bits, k, lookup_bits, seed of synth_paillier_inputs
SHAPES = (("encrypt", 128, 64, 14, 13, 0x50), ("add", 128, 64, 12, 11, 0x99), ("encrypt_uniform", 128, 64, 15, 14, 0x51))
KIND_ID = {"encrypt": 0, "add": 1, "encrypt_uniform": 2}


def inputs(kind: str, bits: int, seed: int):
    """-> n, g, x, y, res of the oracle's circuit: encrypt (x, y) = (m, r), res = g^m r^n mod n^2; add (x, y) = (c1, c2), res = c1 c2 mod n^2"""
    n, g, m, r = P.synth_paillier_inputs(bits, seed, standard_g=False)
    res = P.paillier_add_native(n, m, r) if kind == "add" else P.paillier_enc_native(n, g, m, r)
    return n, g, m, r, res


def limbs(v: int, count: int, limb_bits: int) -> List[int]:
    return [(v >> (limb_bits * i)) & ((1 << limb_bits) - 1) for i in range(count)]


def statement(kind: str, n: int, g: int, x: int, y: int, res: int, bits: int, W: int) -> List[int]:
    """the public values in the instance column's row order"""
    Ln = bits // W
    vals = limbs(n, Ln, W) + limbs(g, Ln, W)
    if kind == "add":
        vals += limbs(x, Ln, W) + limbs(y, Ln, W)
    return vals + limbs(res, 2 * Ln, W)


def exposed_positions(kind: str, n: int, g: int, x: int, y: int, res: int, bits: int, W: int, lb: int) -> List[int]:
    """stream indices of the exposed cells from a walk of its own over the oracle's cell stream: the four assign_integer at the head put
    their limb cells first and take equally many cells each (n at 0: the first cell of the second block of Ln limb values is g's); res is
    the last assign_integer: the 2 Ln limb cells in front of the final assert_equal_fresh, whose length is 2 + 16 * 2 Ln cells [D]"""
    Ln = bits // W
    adv = P.expand_circuit_cells_wired(kind, n, g, x, y, res, bits, W, lb, full=True)["advice"]
    # one assign_integer block: Ln limb cells, then the range checks; its length is where g's limbs start -- found from the VALUES
    # (distinct random limbs): the first position after n's limbs that holds g's limbs in a row
    g_l = limbs(g, Ln, W)
    stride = next(i for i in range(Ln, len(adv)) if adv[i:i + Ln] == g_l)
    heads = 4 if kind == "add" else 2
    cells = [h * stride + j for h in range(heads) for j in range(Ln)]
    r_l = limbs(res, 2 * Ln, W)
    res_at = len(adv) - (2 + 16 * 2 * Ln) - 2 * stride        # assign_integer of 2 Ln limbs is twice as long as one of Ln
    assert adv[res_at:res_at + 2 * Ln] == r_l and adv[:Ln] == limbs(n, Ln, W)
    return cells + [res_at + j for j in range(2 * Ln)]


def extended_equalities(st, cells: Sequence[int], constants: Sequence[int] = None):
    """the oracle structure's copy constraints + (exposed cell i) == (instance column, row i).  constants: another row order of the
    constants column (each generator numbers the distinct constants in its own walk order) -- rows are renamed through the VALUES"""
    eqs = list(st.equalities)
    if constants is not None:
        row_of = {int(v) % R: i for i, v in enumerate(constants)}
        assert sorted(row_of) == sorted(v % R for v in st.constants)
        cc = st.n_adv + st.n_lk
        ren = lambda cell: (cc, row_of[st.constants[cell[1]] % R]) if cell[0] == cc else cell
        eqs = [(ren(a), ren(b)) for a, b in eqs]
    return eqs + [(st.pos(c), (st.m, i)) for i, c in enumerate(cells)]


def build_pub(kind: str, n: int, g: int, x: int, y: int, res: int, bits: int, W: int, lb: int, k: int, minimum_rows: int = 20):
    """-> (oracle Structure, exposed stream cells, equalities extended by the instance cells, (map_col, map_row) over m + 1 columns)"""
    st = CQ.build(kind, n, g, x, y, res, bits, W, lb, k, minimum_rows=minimum_rows)
    cells = exposed_positions(kind, n, g, x, y, res, bits, W, lb)
    eqs = extended_equalities(st, cells)
    mc, mr = CQ.permutation_from_equalities(eqs, st.m + 1, st.n)
    return st, cells, eqs, (mc, mr)


def reference_maps(st, cells: Sequence[int], constants: Sequence[int]):
    """(map_col, map_row) u32 [m + 1][2^k] of the reference, the constants column in the given row order"""
    return CQ.permutation_from_equalities(extended_equalities(st, cells, constants), st.m + 1, st.n)


def mock_prover_pub(st, eqs, instance_values: Sequence[int]) -> List[str]:
    """oracle.circuit.mock_prover on [columns | instance column] with the extended equalities"""
    cols = CQ.perm_columns(st) + [list(instance_values) + [0] * (st.n - len(instance_values))]
    saved = st.equalities
    st.equalities = eqs
    try:
        return CQ.mock_prover(st, cols)
    finally:
        st.equalities = saved


def instance_eval(k: int, values: Sequence[int], x: int) -> int:
    """sum_i v_i l_i(x), l_i(x) = (x^n - 1)/n w^i / (x - w^i)"""
    n = 1 << k
    w = P.fr_omega(k)
    xn1 = (pow(x, n, R) - 1) % R
    n_inv = pow(n, -1, R)
    acc = 0
    for i, v in enumerate(values):
        wi = pow(w, i, R)
        acc = (acc + v * xn1 % R * n_inv % R * wi % R * pow((x - wi) % R, -1, R)) % R
    return acc


def expected_h_pub(k: int, bf: int, A: int, Lk: int, chunk: int, ev: Dict[str, List[List[int]]], beta: int, gamma: int, y: int, x: int, delta: int,
                   inst_x=None) -> int:
    """oracle.verifier.expected_h with the instance column's value at x as the LAST permuted value (inst_x = None: no instance column,
    the oracle's function itself)"""
    if inst_x is None:
        return V.expected_h(k, bf, A, Lk, chunk, ev, beta, gamma, y, x, delta)
    n = 1 << k
    l0, llast, lblind = V.lagrange_at(k, bf, x)
    lact = (1 - llast - lblind) % R
    acc = 0

    def line(v):
        nonlocal acc
        acc = (acc * y + v) % R

    for j in range(A):
        a0, a1, a2, a3 = ev["advice"][j]
        line(ev["fixed"][j][0] * (a0 + a1 * a2 - a3))
    vals = [ev["advice"][j][0] for j in range(A)] + [ev["lookup_advice"][j][0] for j in range(Lk)] + [ev["fixed"][A][0], inst_x % R]
    m = len(vals)
    S = -(-m // chunk)
    z = ev["perm_z"]
    line(l0 * (1 - z[0][0]))
    line(llast * (z[S - 1][0] * z[S - 1][0] - z[S - 1][0]))
    for j in range(1, S):
        line(l0 * (z[j][0] - z[j - 1][2]))
    cur = beta * x % R
    for j in range(S):
        left, right = z[j][1], z[j][0]
        for c in range(j * chunk, min(m, (j + 1) * chunk)):
            left = left * (vals[c] + beta * ev["sigma"][c][0] + gamma) % R
            right = right * (vals[c] + cur + gamma) % R
            cur = cur * delta % R
        line(lact * (left - right))
    tab = ev["fixed"][A + 1][0]
    for j in range(Lk):
        a = ev["lookup_advice"][j][0]
        zx, zwx = ev["lookup_z"][j]
        ap, ap_prev = ev["perm_inputs"][j]
        sp = ev["perm_tables"][j][0]
        line(l0 * (1 - zx))
        line(llast * (zx * zx - zx))
        line(lact * (zwx * (ap + beta) % R * (sp + gamma) - zx * (a + beta) % R * (tab + gamma)))
        line(l0 * (ap - sp))
        line(lact * (ap - sp) % R * (ap - ap_prev))
    return acc * pow(pow(x, n, R) - 1, -1, R) % R


def replay_challenges_pub(seed: bytes, instance_values: Sequence[int], commitments, evals) -> Dict[str, int]:
    """oracle.verifier.replay_challenges with the statement absorbed after the seed and before the first commitment: each value a scalar
    (tag 2) in its 4 Montgomery words.  With no values this IS the oracle's replay."""
    h = hashlib.blake2b(bytes(seed), digest_size=64, person=b"Halo2-Transcript")
    out: Dict[str, int] = {}
    mont = lambda v: [((v * (1 << 256)) % R >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]

    def words(row):
        return [int(w) for w in (row.reshape(-1) if hasattr(row, "reshape") else row)]

    def point(row):
        h.update(b"\x01" + struct.pack("<8Q", *words(row)))

    def scalars(row):
        w = words(row)
        for i in range(0, len(w), 4):
            h.update(b"\x02" + struct.pack("<4Q", *w[i:i + 4]))

    def draw(name):
        h.update(b"\x00")
        out[name] = int.from_bytes(h.copy().digest(), "little") % R

    for v in instance_values:
        scalars(mont(int(v)))
    for fams, names in V.COMMITMENT_ROUNDS:
        for f in fams:
            for row in commitments[f]:
                point(row)
        for nm in names:
            draw(nm)
    for f in V.EVAL_FAMILIES:
        for row in evals[f]:
            scalars(row)
        if f == "lookup_advice" and "constants" in evals:
            for row in evals["constants"]:
                scalars(row)
    draw("sh_y")
    draw("sh_v")
    for row in commitments["w1"]:
        point(row)
    draw("sh_u")
    return out


def query_layout_pub(A: int, Lk: int, m: int, S: int):
    """the prover's query order (rotation sets as point indices into {x, wx, w^2 x, w^3 x, w^-(bf+1) x, w^-1 x}) with m sigma members,
    m counting the instance column's sigma; the instance column itself is not a member: it is not opened"""
    s0 = [("lookup_advice", i) for i in range(Lk)] + [("fixed", i) for i in range(A + 2)] + [("sigma", i) for i in range(m)] + \
         [("perm_tables", i) for i in range(Lk)] + [("h", 0), ("random", 0)]
    sets = [([0], s0), ([0, 1, 2, 3], [("advice", i) for i in range(A)])]
    if S > 1:
        sets.append(([0, 1, 4], [("perm_z", i) for i in range(S - 1)]))
    sets.append(([0, 1], [("perm_z", S - 1)] + [("lookup_z", i) for i in range(Lk)]))
    sets.append(([0, 5], [("perm_inputs", i) for i in range(Lk)]))
    return sets


def ints_of(cref, a) -> List[List[int]]:
    a = np.asarray(a, dtype=np.uint64)
    flat = cref.fr_mont_to_ints(a.reshape(-1, 4))
    p_ = a.shape[1]
    return [flat[i * p_:(i + 1) * p_] for i in range(a.shape[0])]
