"""CPU: the mix's switch network -- the product's routing (paillier_halo2_amd/mix.py, pz_mix_route) against the
independent restatement of tests/mix_ref.py, both ways round, and the soundness premise: whatever the bits, the network permutes."""
import itertools
import random

import numpy as np
import pytest

from paillier_halo2_amd import mix
from tests import mix_ref as MR


def _perms(K, seed, count=20):
    rng = random.Random(seed)
    out = [list(range(K)), list(range(K - 1, -1, -1))]
    for _ in range(count):
        p = list(range(K))
        rng.shuffle(p)
        out.append(p)
    return out


def _holds(K, perm):
    xs = [1000 + 7 * i for i in range(K)]
    want = [xs[p] for p in perm]
    bits = mix.benes_route(perm)
    assert len(bits) == MR.n_bits(K) and set(bits) <= {0, 1}
    layers = MR.apply(bits, xs)
    assert (layers[-1] if layers else xs) == want                       # the product's router under the reference's network
    assert mix.benes_apply(MR.route(perm), xs) == want                  # the reference's router under the product's network
    assert mix.benes_apply(bits, xs) == want


# ------------------------------------------------------------------------------------------------------------------ routing
@pytest.mark.parametrize("K", [2, 4, 8])
def test_every_permutation_routes(K):
    n = 0
    for perm in itertools.permutations(range(K)):
        _holds(K, list(perm))
        n += 1
    assert n == {2: 2, 4: 24, 8: 40320}[K]


@pytest.mark.parametrize("K", [1, 16, 64, 1024])
def test_random_permutations_route(K):
    for perm in _perms(K, 0x3170 + K):
        _holds(K, perm)


def test_the_network_is_the_pinned_one():
    """layer count, the bit each layer acts on, switch order and partner, written out for K = 8"""
    assert MR.benes_layers(1) == [] and MR.benes_layers(2) == [[(0, 1)]]
    assert mix.layer_bits(8) == [0, 1, 2, 1, 0] and mix.layer_bits(1) == [] and mix.layer_bits(1024) == list(range(10)) + list(range(8, -1, -1))
    L8 = MR.benes_layers(8)
    assert L8[0] == L8[4] == [(0, 1), (2, 3), (4, 5), (6, 7)]
    assert L8[1] == L8[3] == [(0, 2), (1, 3), (4, 6), (5, 7)]
    assert L8[2] == [(0, 4), (1, 5), (2, 6), (3, 7)]
    for K in (2, 8, 64):
        for l, (beta, layer) in enumerate(zip(mix.layer_bits(K), MR.benes_layers(K))):
            assert [mix.switch_index(j, beta) for j, _ in layer] == list(range(K // 2))
    # one set bit moves exactly its switch's two values
    xs = list(range(8))
    for at in range(MR.n_bits(8)):
        bits = [0] * MR.n_bits(8)
        bits[at] = 1
        j, jp = L8[at // 4][at % 4]
        want = list(xs)
        want[j], want[jp] = xs[jp], xs[j]
        assert MR.apply(bits, xs)[-1] == want == mix.benes_apply(bits, xs)


def test_any_bits_give_a_permutation():
    """the soundness premise: a network of conditional swaps permutes whatever its bits are"""
    xs = [10, 11, 12, 13]
    for bits in itertools.product((0, 1), repeat=6):
        assert sorted(MR.apply(bits, xs)[-1]) == xs and mix.benes_apply(bits, xs) == MR.apply(bits, xs)[-1]
    rng = random.Random(0x3171)
    xs = list(range(16))
    seen = set()
    for _ in range(1000):
        bits = [rng.randrange(2) for _ in range(MR.n_bits(16))]
        out = MR.apply(bits, xs)[-1]
        assert sorted(out) == xs and mix.benes_apply(bits, xs) == out
        seen.add(tuple(out))
    assert len(seen) > 900


def test_python_refusals_and_random_permutation():
    for bad in ([0, 0], [0, 2], [1, 2, 0], [0, 1, 2, 4], list(range(2048))):
        with pytest.raises(ValueError):
            mix.benes_route(bad)
    with pytest.raises(ValueError):
        mix.benes_apply([0], [1, 2, 3, 4])
    with pytest.raises(ValueError):
        mix.benes_apply([2], [1, 2])
    assert mix.benes_route([0]) == b"" and mix.benes_apply(b"", [5]) == [5]
    rng = random.Random(0x3172)
    p = mix.random_permutation(64, rand=rng.randrange)
    assert sorted(p) == list(range(64)) and p != list(range(64))
    assert sorted(mix.random_permutation(8)) == list(range(8))          # the system's generator
    draws = iter([0, 0, 0])                                             # Fisher-Yates from the top: rand(4), rand(3), rand(2)
    assert mix.random_permutation(4, rand=lambda k: next(draws)) == [1, 2, 3, 0]


# ------------------------------------------------------------------------------------------------------------------ pz_mix_route
@pytest.fixture(scope="module")
def L():
    import paillier_halo2_amd as pz

    pz.build()
    return pz.lib()


def _native(L, perm):
    p = np.array(perm, dtype=np.uint32)
    bits = np.full(19 * 512 + 1, 7, dtype=np.uint8)                    # the largest network's bits and one byte more
    rc = L.pz_mix_route(len(perm), p.ctypes.data, bits.ctypes.data)
    return rc, bits


def test_native_route_equals_the_python_one(L):
    import paillier_halo2_amd as pz

    for K in (1, 2, 4, 8, 16, 64, 1024):
        perms = _perms(K, 0x3170 + K)
        if K in (4, 8):
            perms += [list(p) for p in itertools.islice(itertools.permutations(range(K)), 0, 5040, 7)]
        for perm in perms:
            rc, bits = _native(L, perm)
            assert rc == 0 and bits[: MR.n_bits(K)].tobytes() == mix.benes_route(perm)
            assert K > 1 or bits[0] == 7
        assert pz.Engine.mix_route(perms[-1]).tobytes() == mix.benes_route(perms[-1])


def test_native_route_refusals(L):
    from paillier_halo2_amd import _lib

    for bad in ([0, 0, 1, 2], [0, 1, 2, 4], [0, 1, 2], [2, 0, 1], list(range(2048)), []):
        rc, bits = _native(L, bad)
        assert rc == _lib.PZ_ERR_INVALID and (bits == 7).all()
    p = np.arange(4, dtype=np.uint32)
    assert L.pz_mix_route(4, None, np.zeros(6, dtype=np.uint8).ctypes.data) == _lib.PZ_ERR_INVALID
    assert L.pz_mix_route(4, p.ctypes.data, None) == _lib.PZ_ERR_INVALID
    assert L.pz_mix_route(1, p.ctypes.data, None) == 0


# ------------------------------------------------------------------------------------------------------------------ layout, mask, structure
from oracle import pyref as P  # noqa: E402
from tests import decrypt_ref as DR  # noqa: E402

S4 = dict(bits=128, W=64, lb=10, k=13, K=4)


def _mix_inputs(bits, K, seed):
    """encryptions under the fixture key; r: 1, n - 1, then random; a seeded permutation routed by the reference"""
    rng = random.Random(seed)
    key = DR.key(bits)
    n, g = key[0], key[1]
    cts = [P.paillier_enc_native(n, g, rng.randrange(n), rng.randrange(1, n)) for _ in range(K)]
    rs = [[1, n - 1][i] if i < 2 else rng.randrange(1, n) for i in range(K)]
    perm = list(range(K))
    rng.shuffle(perm)
    return n, cts, rs, perm


def _trace(n, cts, rs, sw, bits, W, forge=None):
    return MR.mix_trace(n, cts, sw, rs, forge=forge, limb_bits=W, limbs=2 * (bits // W))


@pytest.mark.parametrize("bits,W,lb,K", [(128, 64, 10, 1), (128, 64, 10, 2), (128, 64, 10, 4), (264, 88, 11, 2)])
def test_layout_counts_and_offsets_equal_the_reference_stream(bits, W, lb, K):
    from paillier_halo2_amd import layout

    n, cts, rs, perm = _mix_inputs(bits, K, 0x3190 + K)
    tr = _trace(n, cts, rs, MR.route(perm), bits, W)
    n2 = n * n
    assert tr.mixed == [cts[p] * pow(r, n, n2) % n2 for p, r in zip(perm, rs)]
    nr = MR.n_steps_r(n)
    assert len(MR.records(tr)) == K * (nr + 1)
    adv, lk, seg = MR.mix_cells(n, cts, rs, tr.mixed, bits, W, lb, tr)
    Ln = bits // W
    cc = layout.circuit_cells("mix", Ln, W, lb, count=K, n_steps_r=nr)
    assert (cc.advice, cc.lookup) == (len(adv), len(lk)) and seg["satisfied"]
    for name in ("assign_n", "assign_cts", "assign_rs", "square", "refresh", "load_zero", "network", "outputs", "results", "end"):
        assert cc.seg[name] == seg[name], name
    assert MR.mix_gate_mask(K, bits, W, lb, nr).shape[0] == len(adv)
    mm = layout.mul_mod_cells(2 * Ln, W, lb)
    assert cc.seg["outputs"][0] - cc.seg["network"][0] == MR.n_bits(K) * (4 + 16 * 2 * Ln)           # a switch: 4 + 16 L cells
    assert cc.seg["results"][0] - cc.seg["outputs"][0] == K * (2 + (nr + 1) * mm.advice)
    assert 4 + 16 * 2 * Ln < mm.advice                                                               # below one block per switch


@pytest.mark.parametrize("bits,W,lb,K", [(128, 64, 10, 1), (128, 64, 10, 4), (264, 88, 11, 2)])
def test_python_structure_gate_mask_and_public_cells(bits, W, lb, K):
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    n, cts, rs, perm = _mix_inputs(bits, K, 0x31A0 + K)
    nr = MR.n_steps_r(n)
    sa = CS.stream_structure("mix", bits, W, lb, exp_r=n, count=K)
    assert np.array_equal(sa.gate_mask, MR.mix_gate_mask(K, bits, W, lb, nr))
    Ln = bits // W
    cc = layout.circuit_cells("mix", Ln, W, lb, count=K, n_steps_r=nr)
    assert (sa.n_cells, sa.n_steps_g, sa.n_steps_r) == (cc.advice, 0, nr)
    wide = layout.assign_cells(2 * Ln, W, lb)[0]
    per = wide + layout.assert_equal_cells(2 * Ln)
    want = list(range(Ln)) + [cc.seg["assign_cts"][0] + i * wide + j for i in range(K) for j in range(2 * Ln)] + \
        [cc.seg["results"][0] + i * per + j for i in range(K) for j in range(2 * Ln)]
    assert sa.public_cells.tolist() == want and len(want) == Ln + 2 * K * 2 * Ln
    tr = _trace(n, cts, rs, MR.route(perm), bits, W)
    adv, _, _ = MR.mix_cells(n, cts, rs, tr.mixed, bits, W, lb, tr)
    assert [adv[c] for c in want] == MR.statement(n, cts, tr.mixed, bits, W)


@pytest.fixture(scope="module")
def s4_columns():
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb, k, K = (S4[f] for f in ("bits", "W", "lb", "k", "K"))
    inp = _mix_inputs(bits, K, 0x31B0)
    sa = CS.stream_structure("mix", bits, W, lb, exp_r=inp[0], count=K)
    return inp, sa, CS.columns(sa, k, lb, device="cpu", expose=True), CS.columns(sa, k, lb, device="cpu")


def _placed(cs, starts, n, cts, rs, tr, expose=True, res=None, instances=None):
    bits, W, lb, k = (S4[f] for f in ("bits", "W", "lb", "k"))
    res = tr.mixed if res is None else res
    adv, lk, _ = MR.mix_cells(n, cts, rs, res, bits, W, lb, tr)
    inst = None
    if expose:
        inst = MR.statement(n, cts, res, bits, W) if instances is None else instances
    return MR.place(adv, lk, starts, cs.n_adv, cs.n_lk, cs.max_rows, k, cs.constants, inst)


def test_reference_stream_satisfies_the_python_structure(s4_columns):
    from paillier_halo2_amd import layout

    (n, cts, rs, perm), sa, (cs, starts), (cs0, starts0) = s4_columns
    bits, W, lb = S4["bits"], S4["W"], S4["lb"]
    assert layout.break_points(sa.gate_mask, cs.max_rows).tolist() == starts[: cs.n_adv_used + 1].tolist()
    assert cs.n_instance == 1 and cs0.n_instance == 0 and cs.m == cs0.m + 1 and cs.n_adv_used >= 2
    table = range(1 << lb)
    check = lambda cols, c=cs: MR.check_columns(c.selectors, c.map_col, c.map_row, table, cols, c.n_lk)
    tr = _trace(n, cts, rs, MR.route(perm), bits, W)
    assert check(_placed(cs, starts, n, cts, rs, tr)) == []
    assert check(_placed(cs0, starts0, n, cts, rs, tr, expose=False), cs0) == []                        # ... and without the instance column
    # another permutation and other r_i on the SAME structure, routed by the product
    tr2 = _trace(n, cts, [rs[2], 5, rs[1], rs[3]], mix.benes_route([3, 2, 1, 0]), bits, W)
    assert tr2.routed == cts[::-1] and check(_placed(cs, starts, n, cts, [rs[2], 5, rs[1], rs[3]], tr2)) == []
    only_copy = lambda bad: bool(bad) and {t for t, _, _ in bad} == {"copy"}
    # a wrong claimed output: only the copy of its assert_equal_fresh's bit to the constant 1 fails
    assert only_copy(check(_placed(cs, starts, n, cts, rs, tr, res=[tr.mixed[0], tr.mixed[1] ^ 2] + tr.mixed[2:])))
    # the statement with two outputs exchanged, and with an input changed
    swapped = [tr.mixed[1], tr.mixed[0]] + tr.mixed[2:]
    assert only_copy(check(_placed(cs, starts, n, cts, rs, tr, instances=MR.statement(n, cts, swapped, bits, W))))
    assert only_copy(check(_placed(cs, starts, n, cts, rs, tr, instances=MR.statement(n, [cts[0] ^ 1] + cts[1:], tr.mixed, bits, W))))


FORGES = [("bit", 1, 0, 2), ("dup", 0, 1), ("src", 1, 2, 1), ("in", 3, 1), ("rn", 1, 1), ("d", 2, 1)]


@pytest.mark.parametrize("forge", FORGES, ids=lambda f: f[0])
def test_forged_edges_fail(s4_columns, forge):
    """every forge is consistent downstream: the claimed outputs are what the forged network and blocks give.  The bit 2 trips
    assert_bit's gate (and, its selects leaving no limbs, the copy into the final block); every other forge a copy constraint alone"""
    (n, cts, rs, perm), sa, (cs, starts), _ = s4_columns
    bits, W, lb = S4["bits"], S4["W"], S4["lb"]
    sw = MR.route(perm)
    honest = _trace(n, cts, rs, sw, bits, W)
    ft = _trace(n, cts, rs, sw, bits, W, forge=forge)
    assert ft.mixed != honest.mixed
    if forge[0] == "dup":
        assert len(set(ft.routed)) == 3 and set(ft.routed) < set(cts)                               # one input twice, one dropped
    bad = MR.check_columns(cs.selectors, cs.map_col, cs.map_row, range(1 << lb), _placed(cs, starts, n, cts, rs, ft), cs.n_lk)
    kinds = {t for t, _, _ in bad}
    assert kinds == ({"gate", "copy"} if forge[0] == "bit" else {"copy"})
    if forge[0] == "bit":
        # with equal inputs at the switch the bit 2 changes no value: assert_bit's gate alone objects
        same = [cts[0], cts[1], cts[0], cts[3]]
        ft2 = _trace(n, same, rs, [0] * 6, bits, W, forge=("bit", 1, 0, 2))
        assert ft2.mixed == _trace(n, same, rs, [0] * 6, bits, W).mixed
        bad = MR.check_columns(cs.selectors, cs.map_col, cs.map_row, range(1 << lb), _placed(cs, starts, n, same, rs, ft2), cs.n_lk)
        assert bad and {t for t, _, _ in bad} == {"gate"}


# ------------------------------------------------------------------------------------------------------------------ statement, arguments
def test_statement_order_and_refusals():
    from paillier_halo2_amd import verifier as PV

    bits, W, K = 128, 64, 4
    Ln = bits // W
    n, cts, rs, perm = _mix_inputs(bits, K, 0x31C0)
    tr = _trace(n, cts, rs, MR.route(perm), bits, W)
    kw = dict(enc_bits=bits, limb_bits=W)
    st = PV.public_inputs("mix", n=n, cts=cts, mixed=tr.mixed, **kw)
    assert st == MR.statement(n, cts, tr.mixed, bits, W) and len(st) == Ln + 2 * K * 2 * Ln
    one = PV.public_inputs("mix", n=n, cts=cts[:1], mixed=tr.mixed[:1], **kw)
    assert one == MR.statement(n, cts[:1], tr.mixed[:1], bits, W) and len(one) == Ln + 4 * Ln
    for bad in (dict(cts=cts, mixed=tr.mixed[:2]),                          # lists of different lengths
                dict(cts=cts[:3], mixed=tr.mixed[:3]),                      # no power of two
                dict(cts=[], mixed=[]),
                dict(cts=cts * 512, mixed=tr.mixed * 512),                  # 2048
                dict(cts=[n * n] + cts[1:], mixed=tr.mixed),                # c_j >= n^2
                dict(cts=cts, mixed=tr.mixed[:3] + [n * n]),                # c'_i >= n^2
                dict(cts=cts, mixed=[0] + tr.mixed[1:]),                    # c'_i = 0: what r_i = 0 leaves
                dict(cts=cts),
                dict(mixed=tr.mixed),
                dict(cts=cts, mixed=tr.mixed, g=n + 1),
                dict(cts=cts, mixed=tr.mixed, c=cts[0]),
                dict(cts=cts, mixed=tr.mixed, total=1),
                dict(cts=cts, mixed=tr.mixed, m=1),
                dict(cts=cts, mixed=tr.mixed, weights=[1] * 4)):
        with pytest.raises(ValueError):
            PV.public_inputs("mix", n=n, **bad, **kw)
    assert PV.public_inputs("mix", n=n, cts=[0] + cts[1:], mixed=tr.mixed, **kw)[Ln:3 * Ln] == [0] * (2 * Ln)    # an INPUT may be 0
    with pytest.raises(ValueError):
        PV.public_inputs("encrypt", n, n + 1, cts[0], mixed=tr.mixed, **kw)


def test_argument_refusals():
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import layout

    n = DR.key(128)[0]
    for K in (None, 0, 3, 6, 2048):
        with pytest.raises(ValueError):
            layout.circuit_cells("mix", 2, 64, 10, count=K, n_steps_r=190)
        with pytest.raises(ValueError):
            CS.stream_structure("mix", 128, 64, 10, exp_r=n, count=K)
    with pytest.raises(ValueError):
        layout.circuit_cells("mix", 2, 64, 10, count=2)                                     # the r^n chain's records are part of the shape
    with pytest.raises(ValueError):
        layout.circuit_cells("mix", 2, 64, 10, count=2, n_steps_g=1, n_steps_r=190)
    with pytest.raises(ValueError):
        layout.circuit_cells("mix", 2, 64, 10, count=2, n_steps_r=190, m_bits=1)
    with pytest.raises(ValueError):
        layout.circuit_cells("mix", 2, 64, 10, count=2, n_steps_r=190, w_bits=1)
    with pytest.raises(ValueError):
        CS.stream_structure("mix", 128, 64, 10, count=2)                                    # no exp_r
    with pytest.raises(ValueError):
        CS.stream_structure("mix", 128, 64, 10, exp_r=n, count=2, m_bits=1)
    with pytest.raises(ValueError):
        CS.stream_structure("encrypt", 128, 64, 10, exp_g=3, exp_r=n, count=2)
