"""CPU: public inputs (one instance column) -- which cells a circuit exposes (pz_circuit_public_cells, host
only; circuit_structure.stream_structure; verifier.public_inputs) against the oracle's walk WITH values, the oracle's MockProver on the
columns + instance column with the extended copy constraints, and the reference's own pieces (tests/public_ref.py) against the oracle."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import circuit as CQ
from oracle import pyref as P
from oracle import verifier as V
from tests import public_ref as PR

R = P.FR_R


@pytest.fixture(scope="module")
def built():
    """per shape: inputs, the oracle structure, the exposed cells, the extended equalities and maps -- computed once, left unchanged"""
    out = {}
    for kind, bits, W, k, lb, seed in PR.SHAPES:
        n, g, x, y, res = PR.inputs(kind, bits, seed)
        out[kind] = (n, g, x, y, res) + PR.build_pub(kind, n, g, x, y, res, bits, W, lb, k)
    return out


@pytest.mark.parametrize("kind,bits,W,k,lb,seed", PR.SHAPES)
def test_public_cell_positions(built, kind, bits, W, k, lb, seed):
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import verifier as PV

    n, g, x, y, res, st, cells, eqs, maps = built[kind]
    Ln = bits // W
    want_count = 6 * Ln if kind == "add" else 4 * Ln
    assert len(cells) == want_count
    if kind == "encrypt":
        assert (cells[0], cells[Ln], cells[2 * Ln]) == (0, 36, 472464)
    sa = CS.stream_structure(kind, bits, W, lb, x, n)
    L = pz.lib()
    npub = C.c_size_t()
    args = (PR.KIND_ID[kind], Ln, W, lb, sa.n_steps_g, sa.n_steps_r)
    assert L.pz_circuit_public_cells(*args, None, 0, C.byref(npub)) == 0 and npub.value == want_count       # count only
    out = np.zeros(want_count, dtype=np.uint64)
    assert L.pz_circuit_public_cells(*args, out.ctypes.data, want_count - 1, C.byref(npub)) == pz._lib.PZ_ERR_CAPACITY
    assert L.pz_circuit_public_cells(*args, out.ctypes.data, want_count, C.byref(npub)) == 0
    assert out.tolist() == cells and sa.public_cells.tolist() == cells
    assert L.pz_circuit_public_cells(3, Ln, W, lb, 0, 0, out.ctypes.data, want_count, C.byref(npub)) == pz._lib.PZ_ERR_INVALID
    # the oracle's advice values at those positions are the limbs of n, g, (c1, c2,) c -- and public_inputs returns them
    vals = PR.statement(kind, n, g, x, y, res, bits, W)
    adv = [st.adv_cols[c][r] for c, r in (st.pos(cell) for cell in cells)]
    assert adv == vals
    got = PV.public_inputs(kind, n, g, res, x, y, enc_bits=bits, limb_bits=W) if kind == "add" else \
        PV.public_inputs(kind, n, g, res, enc_bits=bits, limb_bits=W)
    assert got == vals
    with pytest.raises(ValueError):
        PV.public_inputs(kind, n << 64, g, res, x, y, enc_bits=bits, limb_bits=W)


@pytest.mark.parametrize("kind,bits,W,k,lb,seed", PR.SHAPES)
def test_mock_prover_with_the_instance_column(built, kind, bits, W, k, lb, seed):
    n, g, x, y, res, st, cells, eqs, (mc, mr) = built[kind]
    vals = PR.statement(kind, n, g, x, y, res, bits, W)
    assert PR.mock_prover_pub(st, eqs, vals) == []
    for i in (0, len(vals) - 1):
        bad = list(vals)
        bad[i] += 1
        fails = PR.mock_prover_pub(st, eqs, bad)
        assert fails and all(f.startswith("copy") for f in fails) and any(f.endswith("%d:%d" % (st.m, i)) for f in fails)
    # instance row i lands in the cycle of stream cell i, as the greatest cell of its class
    flat = mc.astype(np.int64) * st.n + mr
    assert np.unique(flat).size == flat.size
    for i, cell in enumerate(cells):
        c, r = st.pos(cell)
        cyc, cur = [], (c, r)
        while True:
            cyc.append(cur)
            cur = (int(mc[cur]), int(mr[cur]))
            if cur == (c, r):
                break
        assert (st.m, i) in cyc and max(cyc) == (st.m, i)
    # untouched outside: every cell of the first m columns that does not map into the instance column keeps its image
    keep = mc[:st.m] < st.m
    assert np.array_equal(mc[:st.m][keep], st.map_col[keep]) and np.array_equal(mr[:st.m][keep], st.map_row[keep])
    assert int((~keep).sum()) == len(cells)


def test_instance_eval_is_the_interpolated_column():
    k = 4
    n = 1 << k
    w = P.fr_omega(k)
    rng = random.Random(0x1d)
    for L in (1, 2, 5, 9):
        vals = [rng.randrange(R) for _ in range(L)]
        coeffs = P.interpolate([pow(w, i, R) for i in range(n)], vals + [0] * (n - L))
        for _ in range(3):
            x = rng.randrange(2, R)
            assert PR.instance_eval(k, vals, x) == P.poly_eval(coeffs, x)
    from paillier_halo2_amd import verifier as PV

    x = rng.randrange(2, R)
    assert PV.instance_eval(k, vals, x) == PR.instance_eval(k, vals, x)


def test_expected_h_pub_without_the_column_is_the_oracles():
    rng = random.Random(0x1e)
    A, Lk, k, bf = 3, 2, 5, 6
    m = A + Lk + 1
    S = -(-m // 2)
    f = lambda cnt, pts: [[rng.randrange(R) for _ in range(pts)] for _ in range(cnt)]
    ev = {"advice": f(A, 4), "lookup_advice": f(Lk, 1), "fixed": f(A + 2, 1), "sigma": f(m + 1, 1), "perm_z": f(S, 3), "lookup_z": f(Lk, 2),
          "perm_inputs": f(Lk, 2), "perm_tables": f(Lk, 1)}
    ch = [rng.randrange(2, R) for _ in range(4)]
    delta = pow(7, 1 << 28, R)
    assert PR.expected_h_pub(k, bf, A, Lk, 2, ev, *ch, delta) == V.expected_h(k, bf, A, Lk, 2, ev, *ch, delta)
    # with the column: the last chunk takes the extra value (m + 1 = 7 columns, 4 sets), so the result moves with it
    ev["perm_z"] = f(S + 1, 3)
    a, b = (PR.expected_h_pub(k, bf, A, Lk, 2, ev, *ch, delta, inst_x=v) for v in (5, 6))
    assert a != b
    # the replay with no statement is the oracle's replay
    com = {nm: np.arange(8 * c, dtype=np.uint64).reshape(c, 8) for nm, c in (("advice", A), ("lookup_advice", Lk), ("perm_inputs", Lk),
           ("perm_tables", Lk), ("perm_z", S), ("lookup_z", Lk), ("random", 1), ("h", 3), ("w1", 1))}
    evw = {nm: np.asarray(v, dtype=object) for nm, v in ev.items()}
    evw = {nm: np.array([[[(x_ >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for x_ in row] for row in v], dtype=np.uint64) for nm, v in ev.items()}
    evw["random"] = np.zeros((1, 1, 4), dtype=np.uint64)
    assert PR.replay_challenges_pub(b"s", [], com, evw) == V.replay_challenges(b"s", com, evw)
    assert PR.replay_challenges_pub(b"s", [1], com, evw) != V.replay_challenges(b"s", com, evw)


def test_python_structure_with_the_instance_column_equals_the_reference(built):
    """circuit_structure.columns(expose=True) on the host: maps equal to the reference's array for array (the add shape; the GPU test
    covers all three with the device generator), selectors and everything else as without the column"""
    from paillier_halo2_amd import circuit_structure as CS

    kind, bits, W, k, lb, seed = PR.SHAPES[1]
    n, g, x, y, res, st, cells, eqs, (mc, mr) = built[kind]
    sa = CS.stream_structure(kind, bits, W, lb, x, n)
    cs0, starts0 = CS.columns(sa, k, lb, device="cpu")
    cs, starts = CS.columns(sa, k, lb, device="cpu", expose=True)
    assert (cs.n_instance, cs.n_public, cs.m) == (1, len(cells), cs0.m + 1) and (cs0.n_instance, cs0.n_public) == (0, 0)
    assert cs.public_cells == [st.pos(c) for c in cells]
    assert np.array_equal(cs.selectors, cs0.selectors) and np.array_equal(starts, starts0) and list(cs.constants) == list(cs0.constants)
    want_c, want_r = PR.reference_maps(st, cells, cs.constants)      # (the constants column in the product's row order)
    assert np.array_equal(cs.map_col.view(np.uint32), want_c) and np.array_equal(cs.map_row.view(np.uint32), want_r)
    # and without the column nothing moved: the first m columns differ only where a class's last cell now maps to its instance cell
    moved = cs.map_col.view(np.uint32)[:cs0.m] != cs0.map_col.view(np.uint32)
    assert int(moved.sum()) == len(cells) and (cs.map_col.view(np.uint32)[:cs0.m][moved] == cs0.m).all()
