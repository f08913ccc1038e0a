"""CPU: the ballot circuit (kind 6 / "ballot") -- cell totals and segment offsets against the reference stream,
the statement's order and refusals, and the Python structure generator held against the independent restatement of
tests/ballot_ref.py by a column-form satisfiability check, with the four forged edges.  No device."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import ballot_ref as BR

S1B = dict(bits=128, W=64, lb=10, k=13, K=2, b=1)


def _inputs(bits, K, b, seed):
    rng = random.Random(seed)
    n, g = P.synth_paillier_inputs(bits, seed)[:2]
    special = [0, (1 << b) - 1, 1 << (b - 1)]            # zero, all ones, a lone top bit
    ms = [special[i] if i < 3 else rng.randrange(1 << b) for i in range(K)]
    rs = [[1, n - 1][i] if i < 2 else rng.randrange(1, n) for i in range(K)]
    return n, g, ms, rs


@pytest.mark.parametrize("bits,W,lb", [(128, 64, 10), (264, 88, 11)])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("b", [1, 2, 64])
def test_layout_counts_and_offsets_equal_the_reference_stream(bits, W, lb, K, b):
    from paillier_halo2_amd import layout

    n, g, ms, rs = _inputs(bits, K, b, 0x6a11 + 16 * K + b)
    tr = BR.ballot_trace(n, g, ms, rs, b)
    n2 = n * n
    assert tr.cts == [pow(g, m, n2) * pow(r, n, n2) % n2 for m, r in zip(ms, rs)]
    nr = BR.n_steps_r(n)
    assert len(BR.records(tr)) == K * (2 * b + nr + 1)
    adv, lk, seg = BR.ballot_cells(n, g, ms, rs, tr.cts, b, bits, W, lb)
    Ln = bits // W
    cc = layout.circuit_cells("ballot", Ln, W, lb, count=K, m_bits=b, n_steps_r=nr)
    assert (cc.advice, cc.lookup) == (len(adv), len(lk)) and seg["satisfied"]
    names = ["assign_n", "assign_g", "messages", "assign_rs", "square", "refresh", "load_zero", "entries", "results", "end"]
    for name in names + (["sum"] if K >= 2 else []):
        assert cc.seg[name] == seg[name], name
    assert ("sum" in cc.seg) == ("sum" in seg) == (K >= 2)
    assert cc.seg["assign_rs"][0] - cc.seg["messages"][0] == K + (1 + 3 * (K - 1) if K >= 2 else 0)
    assert BR.ballot_gate_mask(K, b, bits, W, lb, nr).shape[0] == len(adv)
    # the closed form of one entry: 2 b + nr + 1 blocks, the select cells, two [1, 0] pairs and num_to_bits
    mm = layout.mul_mod_cells(2 * Ln, W, lb)
    assert cc.seg["results"][0] - cc.seg["entries"][0] == K * ((2 * b + nr + 1) * mm.advice + b * 16 * Ln + 4 + 7 * b - 2)


@pytest.mark.parametrize("bits,W,lb,K,b", [(128, 64, 10, 1, 1), (128, 64, 10, 3, 2), (264, 88, 11, 2, 1)])
def test_python_structure_gate_mask_and_public_cells(bits, W, lb, K, b):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    n, g, ms, rs = _inputs(bits, K, b, 0x6a21 + K)
    nr = BR.n_steps_r(n)
    sa = CS.stream_structure("ballot", bits, W, lb, exp_r=n, count=K, m_bits=b)
    assert np.array_equal(sa.gate_mask, BR.ballot_gate_mask(K, b, bits, W, lb, nr))
    Ln = bits // W
    cc = layout.circuit_cells("ballot", Ln, W, lb, count=K, m_bits=b, n_steps_r=nr)
    assert (sa.n_cells, sa.n_steps_g, sa.n_steps_r) == (cc.advice, 2 * b, nr)
    per = layout.assign_cells(2 * Ln, W, lb)[0] + layout.assert_equal_cells(2 * Ln)
    want = list(range(Ln)) + [cc.seg["assign_g"][0] + j for j in range(Ln)] + \
        [cc.seg["results"][0] + i * per + j for i in range(K) for j in range(2 * Ln)]
    if K >= 2:
        want.append(cc.seg["assign_rs"][0] - 1)             # the last cell of the sum
    assert sa.public_cells.tolist() == want and len(want) == 2 * Ln + K * 2 * Ln + (K >= 2)
    # ... and those cells hold the statement in the reference stream
    tr = BR.ballot_trace(n, g, ms, rs, b)
    adv, _, _ = BR.ballot_cells(n, g, ms, rs, tr.cts, b, bits, W, lb)
    assert [adv[c] for c in want] == BR.statement(n, g, tr.cts, sum(ms) if K >= 2 else None, bits, W)


@pytest.fixture(scope="module")
def s1b_columns():
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k, K, b = (S1B[f] for f in ("bits", "W", "lb", "k", "K", "b"))
    n, g, ms, rs = _inputs(bits, K, b, 0x6a31)
    sa = CS.stream_structure("ballot", bits, W, lb, exp_r=n, count=K, m_bits=b)
    return (n, g, ms, rs), sa, CS.columns(sa, k, lb, device="cpu", expose=True), CS.columns(sa, k, lb, device="cpu")


def _placed(cs, starts, inp, trace=None, expose=True, res=None, instances=None):
    bits, W, lb, k, b = (S1B[f] for f in ("bits", "W", "lb", "k", "b"))
    n, g, ms, rs = inp
    tr = BR.ballot_trace(n, g, ms, rs, b) if trace is None else trace
    res = tr.cts if res is None else res
    adv, lk, _ = BR.ballot_cells(n, g, ms, rs, res, b, bits, W, lb, tr)
    inst = None
    if expose:
        inst = BR.statement(n, g, res, tr.total, bits, W) if instances is None else instances
    return BR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, inst)


def test_reference_stream_satisfies_the_python_structure(s1b_columns):
    from paillier_halo2_amd import layout

    inp, sa, (cs, starts), (cs0, starts0) = s1b_columns
    lb = S1B["lb"]
    assert inp[2] == [0, 1]
    assert layout.break_points(sa.gate_mask, cs.max_rows).tolist() == starts[: cs.n_adv_used + 1].tolist()
    assert cs.n_instance == 1 and cs0.n_instance == 0 and cs.m == cs0.m + 1 and cs.n_adv_used >= 2     # break points are crossed
    table = range(1 << lb)
    check = lambda cols, c=cs: BR.check_columns(c.selectors, c.map_col, c.map_row, table, cols, c.n_lk)
    assert check(_placed(cs, starts, inp)) == []
    assert check(_placed(cs0, starts0, inp, expose=False), cs0) == []                                  # ... and without the instance column
    # another ballot of the same key on the SAME structure
    n, g, ms, rs = inp
    assert check(_placed(cs, starts, (n, g, [1, 1], [rs[1], 5]))) == []
    only_copy = lambda bad: bool(bad) and {t for t, _, _ in bad} == {"copy"}
    # a wrong claimed ciphertext: only the copy of its assert_equal_fresh's bit to the constant 1 fails
    tr = BR.ballot_trace(n, g, ms, rs, S1B["b"])
    assert only_copy(check(_placed(cs, starts, inp, res=[tr.cts[0], tr.cts[1] ^ 2])))
    # a statement total changed by one
    inst = BR.statement(n, g, tr.cts, tr.total + 1, S1B["bits"], S1B["W"])
    assert only_copy(check(_placed(cs, starts, inp, instances=inst)))


@pytest.mark.parametrize("forge", [("exp", 0, 1), ("base", 1, 1), ("rn", 0, 1), ("sum", 1)], ids=lambda f: f[0])
def test_forged_edges_fail(s1b_columns, forge):
    """every forge is consistent downstream: the claimed ciphertexts are what the forged chains give"""
    inp, sa, (cs, starts), _ = s1b_columns
    n, g, ms, rs = inp
    honest = BR.ballot_trace(n, g, ms, rs, S1B["b"])
    ft = BR.ballot_trace(n, g, ms, rs, S1B["b"], forge=forge)
    assert (ft.cts != honest.cts) == (forge[0] != "sum") and (ft.total != honest.total) == (forge[0] == "sum")
    bad = BR.check_columns(cs.selectors, cs.map_col, cs.map_row, range(1 << S1B["lb"]), _placed(cs, starts, inp, trace=ft), cs.n_lk)
    kinds = {t for t, _, _ in bad}
    assert kinds == ({"gate"} if forge[0] == "sum" else {"copy"})       # the sum's own gate objects; elsewhere a copy constraint


def test_statement_order_and_refusals():
    from paillier_halo2_amd import verifier as PV

    bits, W, K, b = 128, 64, 3, 2
    Ln = bits // W
    n, g, ms, rs = _inputs(bits, K, b, 0x6a41)
    tr = BR.ballot_trace(n, g, ms, rs, b)
    kw = dict(enc_bits=bits, limb_bits=W)
    st = PV.public_inputs("ballot", n=n, g=g, cts=tr.cts, total=sum(ms), **kw)
    assert st == BR.statement(n, g, tr.cts, sum(ms), bits, W) and len(st) == 2 * Ln + K * 2 * Ln + 1 and st[-1] == sum(ms)
    one = PV.public_inputs("ballot", n=n, g=g, cts=tr.cts[:1], **kw)
    assert one == BR.statement(n, g, tr.cts[:1], None, bits, W) and len(one) == 2 * Ln + 2 * Ln
    for bad in (dict(cts=tr.cts[:1], total=ms[0]),               # a total with K = 1 would expose the message
                dict(cts=tr.cts),                                # a total missing with K >= 2
                dict(cts=[n * n] + tr.cts[1:], total=1),         # c >= n^2
                dict(cts=[], total=None),
                dict(total=1),                                   # no ciphertexts
                dict(cts=tr.cts, total=-1),
                dict(cts=tr.cts, total=1, c=tr.cts[0]),          # no single result
                dict(cts=tr.cts, total=1, m=1),
                dict(cts=tr.cts, total=1, weights=[1, 1, 1])):
        with pytest.raises(ValueError):
            PV.public_inputs("ballot", n=n, g=g, **bad, **kw)
    with pytest.raises(ValueError):
        PV.public_inputs("ballot", n=n, g=None, cts=tr.cts, total=1, **kw)
    with pytest.raises(ValueError):
        PV.public_inputs("encrypt", n, g, tr.cts[0], total=1, **kw)


def test_argument_refusals():
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    n = P.synth_paillier_inputs(128, 3)[0]
    for K, b in ((None, 1), (0, 1), (1025, 1), (2, None), (2, 0), (2, 65)):
        with pytest.raises(ValueError):
            layout.circuit_cells("ballot", 2, 64, 10, count=K, m_bits=b, n_steps_r=190)
        with pytest.raises(ValueError):
            CS.stream_structure("ballot", 128, 64, 10, exp_r=n, count=K, m_bits=b)
    with pytest.raises(ValueError):
        layout.circuit_cells("ballot", 2, 64, 10, count=2, m_bits=1)                       # the r^n chain's records are part of the shape
    with pytest.raises(ValueError):
        layout.circuit_cells("ballot", 2, 64, 10, n_steps_g=3, n_steps_r=190, count=2, m_bits=1)
    with pytest.raises(ValueError):
        layout.circuit_cells("ballot", 2, 64, 10, count=2, m_bits=1, w_bits=1, n_steps_r=190)
    with pytest.raises(ValueError):
        CS.stream_structure("ballot", 128, 64, 10, count=2, m_bits=1)                      # no exp_r
    for kind in ("encrypt", "encrypt_uniform", "add", "decrypt"):
        with pytest.raises(ValueError):
            layout.circuit_cells(kind, 2, 64, 10, m_bits=1)
    for kind, extra in (("tally", dict(count=3)), ("wtally", dict(count=3, w_bits=2)), ("add", {})):
        with pytest.raises(ValueError):
            layout.circuit_cells(kind, 2, 64, 10, m_bits=1, **extra)
        with pytest.raises(ValueError):
            CS.stream_structure(kind, 128, 64, 10, m_bits=1, **extra)
