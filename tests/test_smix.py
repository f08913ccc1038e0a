"""CPU: the short-randomness mix (kind 10 / "smix") -- the scheme in Python integers (a mixed sballot decrypts
to what its source held, with randomness r_pi(i) h^s_i), cell totals and segment offsets against the reference stream, the statement's
order and refusals, and the Python structure generator held against the independent restatement of tests/smix_ref.py by a column-form
satisfiability check and by the MockProver analogue of oracle/circuit.py, with the eight forged edges.  No device."""
import ctypes as C
import math
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import smix_ref as XR

S4 = dict(bits=128, W=64, lb=10, k=13, K=4, sl=1)


def _prime_3mod4(start: int) -> int:
    from paillier_halo2_amd import keys

    x = start - start % 4 + 3
    while not keys._is_prime(x):
        x += 4
    return x


def _key(bits: int):
    if bits == 128:
        return XR.SAFE_P, XR.SAFE_Q
    assert bits == 264
    return _prime_3mod4((3 << 130) + 12345), _prime_3mod4((3 << 130) + (1 << 100))


def _unit(rng, n):
    while True:
        x = rng.randrange(2, n)
        if math.gcd(x, n) == 1:
            return x


def _inputs(bits, K, s_bits, seed):
    """sballots under a synthetic key of the size; s: 0, all ones, a lone top bit, then random; a seeded permutation"""
    rng = random.Random(seed)
    n, g = P.synth_paillier_inputs(bits, seed)[:2]
    hs = XR.djn_hs(n, _unit(rng, n))
    cts = [XR.encrypt(n, g, hs, rng.randrange(1 << 16), rng.randrange(1 << s_bits)) for _ in range(K)]
    special = [0, (1 << s_bits) - 1, 1 << (s_bits - 1)]
    ss = [special[i] if i < 3 else rng.randrange(1 << s_bits) for i in range(K)]
    perm = list(range(K))
    rng.shuffle(perm)
    return n, hs, cts, ss, perm


def _trace(n, hs, cts, ss, sw, bits, W, sl, forge=None):
    return XR.smix_trace(n, hs, cts, sw, ss, sl * W, forge=forge, limb_bits=W, limbs=2 * (bits // W))


# ------------------------------------------------------------------------------------------------------------------ the scheme
@pytest.mark.parametrize("bits", [128, 264])
def test_a_mixed_sballot_decrypts_to_its_source_with_randomness_r_h_to_the_s(bits):
    p, q = _key(bits)
    assert p % 4 == q % 4 == 3 and p != q
    n = p * q
    assert n.bit_length() == bits
    n2, g = n * n, n + 1
    rng = random.Random(0x5c01 + bits)
    x = _unit(rng, n)
    h, hs = XR.djn_h(n, x), XR.djn_hs(n, x)
    K, s_bits = 4, 40
    ms = [rng.randrange(1 << 16) for _ in range(K)]
    s0 = [rng.randrange(1 << s_bits) for _ in range(K)]
    cts = [XR.encrypt(n, g, hs, m, s) for m, s in zip(ms, s0)]
    ss = [0, (1 << s_bits) - 1, 1 << (s_bits - 1), rng.randrange(1 << s_bits)]
    perm = [2, 0, 3, 1]
    tr = XR.smix_trace(n, hs, cts, XR.route(perm), ss, s_bits)
    assert tr.routed == [cts[j] for j in perm]
    assert tr.mixed == [cts[j] * pow(hs, s, n2) % n2 for j, s in zip(perm, ss)]
    assert len(XR.records(tr)) == K * XR.per_output(s_bits)
    for i, c in enumerate(tr.mixed):
        m_src, r_src = XR.decrypt(p, q, g, cts[perm[i]])
        m_out, r_out = XR.decrypt(p, q, g, c)
        assert m_out == m_src == ms[perm[i]]                          # Dec(c'_i) = Dec(c_pi(i))
        assert r_out == r_src * pow(h, ss[i], n) % n                  # the recovered randomness is r_pi(i) h^s_i mod n
    assert tr.mixed[0] == cts[perm[0]]                                # s = 0 re-randomises nothing: the circuit does not refuse it


# ------------------------------------------------------------------------------------------------------------------ layout, mask, structure
@pytest.mark.parametrize("bits,W,lb,K,sl", [(128, 64, 10, 1, 1), (128, 64, 10, 2, 2), (128, 64, 10, 4, 1), (264, 88, 11, 2, 1)])
def test_layout_counts_and_offsets_equal_the_reference_stream(bits, W, lb, K, sl):
    from paillier_halo2_amd import _lib, layout

    s_bits = sl * W
    n, hs, cts, ss, perm = _inputs(bits, K, s_bits, 0x5c10 + 8 * K + sl)
    tr = _trace(n, hs, cts, ss, XR.route(perm), bits, W, sl)
    n2 = n * n
    assert tr.mixed == [cts[j] * pow(hs, s, n2) % n2 for j, s in zip(perm, ss)]
    adv, lk, seg = XR.smix_cells(n, hs, cts, ss, tr.mixed, sl, bits, W, lb, tr)
    Ln = bits // W
    cc = layout.circuit_cells("smix", Ln, W, lb, count=K, s_limbs=sl)
    assert (cc.advice, cc.lookup) == (len(adv), len(lk)) and seg["satisfied"]
    for name in ("assign_n", "assign_hs", "assign_cts", "assign_ss", "square", "refresh", "load_zero", "network", "outputs", "results", "end"):
        assert cc.seg[name] == seg[name], name
    assert XR.smix_gate_mask(K, sl, bits, W, lb).shape[0] == len(adv)
    mm = layout.mul_mod_cells(2 * Ln, W, lb)
    assert cc.seg["outputs"][0] - cc.seg["network"][0] == XR.n_bits(K) * (4 + 16 * 2 * Ln)
    per = XR.per_output(s_bits)
    assert cc.seg["results"][0] - cc.seg["outputs"][0] == K * (2 + sl * (7 * W - 2) + s_bits * 16 * Ln + per * mm.advice)
    assert cc.lookup - cc.seg["outputs"][1] == K * per * mm.lookup + K * layout.assign_cells(2 * Ln, W, lb)[1]
    # the native cell counts are host logic: no device
    a, l = C.c_size_t(), C.c_size_t()
    assert _lib.lib().pz_smix_cells(Ln, W, lb, K, sl, C.byref(a), C.byref(l)) == 0
    assert (a.value, l.value) == (len(adv), len(lk))


@pytest.mark.parametrize("bits,W,lb,K,sl", [(128, 64, 10, 1, 1), (128, 64, 10, 4, 2), (264, 88, 11, 2, 1)])
def test_python_structure_gate_mask_and_public_cells(bits, W, lb, K, sl):
    from paillier_halo2_amd import _lib, layout
    from paillier_halo2_amd import circuit_structure as CS

    s_bits = sl * W
    n, hs, cts, ss, perm = _inputs(bits, K, s_bits, 0x5c20 + K)
    sa = CS.stream_structure("smix", bits, W, lb, count=K, s_limbs=sl)
    assert np.array_equal(sa.gate_mask, XR.smix_gate_mask(K, sl, bits, W, lb))
    Ln = bits // W
    cc = layout.circuit_cells("smix", Ln, W, lb, count=K, s_limbs=sl)
    assert (sa.n_cells, sa.n_steps_g, sa.n_steps_r) == (cc.advice, 0, 2 * s_bits)
    want = XR.public_cells(K, sl, bits, W, lb)
    wide = layout.assign_cells(2 * Ln, W, lb)[0]
    per = wide + layout.assert_equal_cells(2 * Ln)
    assert want == list(range(Ln)) + [cc.seg["assign_hs"][0] + j for j in range(2 * Ln)] + \
        [cc.seg["assign_cts"][0] + i * wide + j for i in range(K) for j in range(2 * Ln)] + \
        [cc.seg["results"][0] + i * per + j for i in range(K) for j in range(2 * Ln)]
    assert sa.public_cells.tolist() == want and len(want) == Ln + 2 * Ln + 2 * K * 2 * Ln
    # ... and those cells hold the statement in the reference stream
    tr = _trace(n, hs, cts, ss, XR.route(perm), bits, W, sl)
    adv, _, _ = XR.smix_cells(n, hs, cts, ss, tr.mixed, sl, bits, W, lb, tr)
    assert [adv[c] for c in want] == XR.statement(n, hs, cts, tr.mixed, bits, W)
    # the native statement cells are host logic: no device
    out = np.zeros(len(want) + 4, dtype=np.uint64)
    npub = C.c_size_t()
    assert _lib.lib().pz_smix_public_cells(Ln, W, lb, K, sl, C.c_void_p(out.ctypes.data), out.shape[0], C.byref(npub)) == 0
    assert out[: npub.value].tolist() == want


@pytest.fixture(scope="module")
def s4_columns():
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k, K, sl = (S4[f] for f in ("bits", "W", "lb", "k", "K", "sl"))
    inp = _inputs(bits, K, sl * W, 0x5c30)
    sa = CS.stream_structure("smix", bits, W, lb, count=K, s_limbs=sl)
    return inp, sa, CS.columns(sa, k, lb, device="cpu", expose=True), CS.columns(sa, k, lb, device="cpu")


def _placed(cs, starts, n, hs, cts, ss, tr, expose=True, res=None, instances=None):
    bits, W, lb, k, sl = (S4[f] for f in ("bits", "W", "lb", "k", "sl"))
    res = tr.mixed if res is None else res
    adv, lk, _ = XR.smix_cells(n, hs, cts, ss, res, sl, bits, W, lb, tr)
    inst = None
    if expose:
        inst = XR.statement(n, hs, cts, res, bits, W) if instances is None else instances
    return XR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, inst)


def test_reference_stream_satisfies_the_python_structure(s4_columns):
    from paillier_halo2_amd import layout, mix

    (n, hs, cts, ss, perm), sa, (cs, starts), (cs0, starts0) = s4_columns
    bits, W, lb, K, sl = (S4[f] for f in ("bits", "W", "lb", "K", "sl"))
    assert layout.break_points(sa.gate_mask, cs.max_rows).tolist() == starts[: cs.n_adv_used + 1].tolist()
    assert cs.n_instance == 1 and cs0.n_instance == 0 and cs.m == cs0.m + 1 and cs.n_adv_used >= 2
    table = range(1 << lb)
    check = lambda cols, c=cs: XR.check_columns(c.selectors, c.map_col, c.map_row, table, cols, c.n_lk)
    tr = _trace(n, hs, cts, ss, XR.route(perm), bits, W, sl)
    assert check(_placed(cs, starts, n, hs, cts, ss, tr)) == []
    assert XR.mock_prover(cs.selectors, cs.map_col, cs.map_row, _placed(cs, starts, n, hs, cts, ss, tr), cs.n_lk, S4["k"], lb) == []
    assert check(_placed(cs0, starts0, n, hs, cts, ss, tr, expose=False), cs0) == []                    # ... and without the instance column
    # ANOTHER key (n, hs), another permutation routed by the product and other s_i on the SAME structure: only the key's size shapes it
    n_, hs_, cts_, ss_, _ = _inputs(bits, K, sl * W, 0x5c31)
    assert n_ != n and hs_ != hs
    tr2 = _trace(n_, hs_, cts_, ss_[::-1], mix.benes_route([3, 2, 1, 0]), bits, W, sl)
    assert tr2.routed == cts_[::-1] and check(_placed(cs, starts, n_, hs_, cts_, ss_[::-1], tr2)) == []
    only_copy = lambda bad: bool(bad) and {t for t, _, _ in bad} == {"copy"}
    # a wrong claimed output: only the copy of its assert_equal_fresh's bit to the constant 1 fails
    assert only_copy(check(_placed(cs, starts, n, hs, cts, ss, tr, res=[tr.mixed[0], tr.mixed[1] ^ 2] + tr.mixed[2:])))
    # the statement with two outputs exchanged, with an input changed, and with hs changed
    swapped = [tr.mixed[1], tr.mixed[0]] + tr.mixed[2:]
    assert only_copy(check(_placed(cs, starts, n, hs, cts, ss, tr, instances=XR.statement(n, hs, cts, swapped, bits, W))))
    assert only_copy(check(_placed(cs, starts, n, hs, cts, ss, tr, instances=XR.statement(n, hs, [cts[0] ^ 1] + cts[1:], tr.mixed, bits, W))))
    assert only_copy(check(_placed(cs, starts, n, hs, cts, ss, tr, instances=XR.statement(n, hs ^ 1, cts, tr.mixed, bits, W))))


FORGES = [("bit", 1, 0, 2), ("dup", 0, 1), ("src", 1, 2, 1), ("in", 3, 1), ("s", 3, 6), ("base", 1, 1), ("hss", 1, 1), ("d", 2, 1)]


@pytest.mark.parametrize("forge", FORGES, ids=lambda f: f[0])
def test_forged_edges_fail(s4_columns, forge):
    """every forge is consistent downstream: the claimed outputs are what the forged network, chains and blocks give.  The bit 2 trips
    assert_bit's gate (and, its selects leaving no limbs, the copy into the final block); every other forge a copy constraint alone"""
    (n, hs, cts, ss, perm), sa, (cs, starts), _ = s4_columns
    bits, W, lb, sl = (S4[f] for f in ("bits", "W", "lb", "sl"))
    sw = XR.route(perm)
    honest = _trace(n, hs, cts, ss, sw, bits, W, sl)
    ft = _trace(n, hs, cts, ss, sw, bits, W, sl, forge=forge)
    assert ft.mixed != honest.mixed
    if forge[0] == "dup":
        assert len(set(ft.routed)) == 3 and set(ft.routed) < set(cts)                               # one input twice, one dropped
    bad = XR.check_columns(cs.selectors, cs.map_col, cs.map_row, range(1 << lb), _placed(cs, starts, n, hs, cts, ss, ft), cs.n_lk)
    kinds = {t for t, _, _ in bad}
    assert kinds == ({"gate", "copy"} if forge[0] == "bit" else {"copy"})
    # the MockProver analogue of oracle/circuit.py rejects the same witness for the same reason
    mock = XR.mock_prover(cs.selectors, cs.map_col, cs.map_row, _placed(cs, starts, n, hs, cts, ss, ft), cs.n_lk, S4["k"], lb)
    assert mock and {m.split()[0] for m in mock} == kinds


# ------------------------------------------------------------------------------------------------------------------ statement, arguments
def test_statement_order_and_refusals():
    from paillier_halo2_amd import verifier as PV

    bits, W, K, sl = 128, 64, 4, 1
    Ln = bits // W
    n, hs, cts, ss, perm = _inputs(bits, K, sl * W, 0x5c40)
    tr = _trace(n, hs, cts, ss, XR.route(perm), bits, W, sl)
    kw = dict(enc_bits=bits, limb_bits=W)
    st = PV.public_inputs("smix", n=n, hs=hs, cts=cts, mixed=tr.mixed, **kw)
    assert st == XR.statement(n, hs, cts, tr.mixed, bits, W) and len(st) == Ln + 2 * Ln + 2 * K * 2 * Ln
    one = PV.public_inputs("smix", n=n, hs=hs, cts=cts[:1], mixed=tr.mixed[:1], **kw)
    assert one == XR.statement(n, hs, cts[:1], tr.mixed[:1], bits, W) and len(one) == Ln + 6 * Ln
    for bad in (dict(hs=hs, cts=cts, mixed=tr.mixed[:2]),                          # lists of different lengths
                dict(hs=hs, cts=cts[:3], mixed=tr.mixed[:3]),                      # no power of two
                dict(hs=hs, cts=[], mixed=[]),
                dict(hs=hs, cts=cts * 512, mixed=tr.mixed * 512),                  # 2048
                dict(hs=0, cts=cts, mixed=tr.mixed),                               # hs = 0
                dict(hs=n * n, cts=cts, mixed=tr.mixed),                           # hs >= n^2
                dict(hs=hs, cts=[n * n] + cts[1:], mixed=tr.mixed),                # c_j >= n^2
                dict(hs=hs, cts=cts, mixed=tr.mixed[:3] + [n * n]),                # c'_i >= n^2
                dict(hs=hs, cts=cts, mixed=[0] + tr.mixed[1:]),                    # c'_i = 0
                dict(cts=cts, mixed=tr.mixed),                                     # no hs
                dict(hs=hs, cts=cts),
                dict(hs=hs, mixed=tr.mixed),
                dict(hs=hs, cts=cts, mixed=tr.mixed, g=n + 1),
                dict(hs=hs, cts=cts, mixed=tr.mixed, c=cts[0]),
                dict(hs=hs, cts=cts, mixed=tr.mixed, total=1),
                dict(hs=hs, cts=cts, mixed=tr.mixed, m=1),
                dict(hs=hs, cts=cts, mixed=tr.mixed, weights=[1] * 4)):
        with pytest.raises(ValueError):
            PV.public_inputs("smix", n=n, **bad, **kw)
    assert PV.public_inputs("smix", n=n, hs=hs, cts=[0] + cts[1:], mixed=tr.mixed, **kw)[3 * Ln:5 * Ln] == [0] * (2 * Ln)   # an INPUT may be 0
    with pytest.raises(ValueError):
        PV.public_inputs("mix", n=n, hs=hs, cts=cts, mixed=tr.mixed, **kw)           # hs is no part of kind 8's statement


def test_argument_refusals():
    from paillier_halo2_amd import _lib, layout
    from paillier_halo2_amd import circuit_structure as CS

    for K, sl in ((None, 1), (0, 1), (3, 1), (6, 1), (2048, 1), (2, None), (2, 0), (2, 5)):
        with pytest.raises(ValueError):
            layout.circuit_cells("smix", 2, 64, 10, count=K, s_limbs=sl)
        with pytest.raises(ValueError):
            CS.stream_structure("smix", 128, 64, 10, count=K, s_limbs=sl)
    with pytest.raises(ValueError):
        layout.circuit_cells("smix", 2, 64, 10, count=2, s_limbs=1, n_steps_g=1)
    with pytest.raises(ValueError):
        layout.circuit_cells("smix", 2, 64, 10, count=2, s_limbs=1, n_steps_r=190)             # the chain's records follow from s_limbs
    with pytest.raises(ValueError):
        layout.circuit_cells("smix", 2, 64, 10, count=2, s_limbs=1, m_bits=1)
    with pytest.raises(ValueError):
        layout.circuit_cells("mix", 2, 64, 10, count=2, n_steps_r=190, s_limbs=1)
    with pytest.raises(ValueError):
        CS.stream_structure("smix", 128, 64, 10, count=2, s_limbs=1, m_bits=1)
    assert layout.circuit_cells("smix", 2, 64, 10, count=2, s_limbs=1, n_steps_r=128).advice == layout.circuit_cells("smix", 2, 64, 10, count=2, s_limbs=1).advice
    # the C ABI's counts: host logic, PZ_ERR_INVALID = -1 for a shape out of range
    L = _lib.lib()
    a, l = C.c_size_t(), C.c_size_t()
    for K, sl in ((0, 1), (3, 1), (2048, 1), (2, 0), (2, 5)):
        assert L.pz_smix_cells(2, 64, 10, K, sl, C.byref(a), C.byref(l)) == -1
    assert L.pz_smix_cells(2, 64, 10, 2, 4, C.byref(a), C.byref(l)) == 0
    # the K3 entry point's refusals that come before the context is looked at: a null pointer
    assert L.pz_paillier_smix(None, 2, 1, 1, None, None, None, None, None, None, None, 0, None) == -1
