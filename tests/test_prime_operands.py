"""CPU: the catalogue and the model of tests/prime_operands.py.  The model of mont_mul asserts its product,
the bound of the running value and the bound of a column's hi inside itself; here it runs over the whole catalogue, the states it
passes through are pinned per modulus class, a seeded random sweep must stay inside them, and every fixture is checked with Python
integers.  The module takes about 70 s on one core of the build machine: 25 s the catalogue, 19 s the random sweep, 13 s prime_setup's
doublings, 11 s the fixtures."""
import math
import random
from collections import defaultdict

import pytest

from tests import prime_operands as PO
from tests import prime_ref as R

# per modulus class: the (out, top_hi, subtraction taken) the catalogue reaches over every limb count and top-limb width, and the
# largest hi after a move.  out = 1 (the bit above the width arrives as the look-ahead's carry, not as the top limb's hi) needs the full
# capacity and a modulus next to R
PLAIN = [(0, 0, 0), (0, 0, 1)]
STATES = {
    "all_ones": (PLAIN + [(0, 1, 1), (1, 0, 1)], 2),
    "pow2_plus1": (PLAIN, 1),
    "minus_2_64_plus1": (PLAIN + [(0, 1, 1), (1, 0, 1)], 2),
    "alt64": (PLAIN, 2),
    "hi32_1": (PLAIN + [(0, 1, 1)], 2),
    "hi32_1_compl": (PLAIN + [(0, 1, 1)], 2),
    "three": (PLAIN, 0),
    "2^64-59": (PLAIN, 1),
    "R-3": (PLAIN + [(0, 1, 1), (1, 0, 1)], 2),
    "random": (PLAIN + [(0, 1, 1)], 2),
}
SWEEP_LIMBS = (1, 2, 16, 17, 32)
SWEEP = 2000


def _key(s):
    return (s.out, s.top_hi, int(s.taken))


@pytest.fixture(scope="module")
def table():
    """class -> (states, largest hi, longest resolve run, longest borrow run) over the whole catalogue; the model asserts every product"""
    states, top = defaultdict(set), defaultdict(lambda: [0, 0, 0])
    count = 0
    for limbs in PO.LIMBS_ALL:
        for name, a, b, c in PO.triples(limbs):
            s = PO.mont_mul_model(a, b, c, limbs)
            cls = name.split("@")[0]
            states[cls].add(_key(s))
            top[cls] = [max(x, y) for x, y in zip(top[cls], (s.max_hi, s.res_run, s.sub_run))]
            count += 1
    return states, top, count


def test_catalogue_covers_every_shape_and_class():
    assert len(PO.SHAPES) == 32 * 6
    seen = set()
    for limbs, tb in PO.SHAPES:
        ms = PO.moduli(limbs, tb)
        seen |= set(ms)
        assert all(c & 1 and c >= 3 and c < 1 << (64 * limbs) for c in ms.values())
        assert all(c.bit_length() == PO.bits_of(limbs, tb) for k, c in ms.items() if k not in ("three", "2^64-59"))
        if tb == 64:
            assert ms["R-3"] == (1 << (64 * limbs)) - 3 and ms["three"] == 3
            c = ms["R-3"]
            A, B = PO.operands_a(c, limbs), PO.operands_b(c, limbs)
            assert all(v < c for v in A.values()) and all(v < 1 << (64 * limbs) for v in B.values())
            assert {"0", "1", "c-1"} <= set(A) and {"0", "R-1", "R/2", "c"} <= set(B)
            E = PO.capacity(limbs)
            assert all("2^(64*%d)" % j in A and "2^(64*%d-1)" % j in A for j in range(E, limbs, E))
    assert seen == set(PO.CLASSES)


def test_state_table_over_the_whole_catalogue(table):
    states, top, count = table
    assert count > 100000
    assert {k: (sorted(v), top[k][0]) for k, v in states.items()} == {k: (sorted(v[0]), v[1]) for k, v in STATES.items()}
    # the ripples: a carry through 14 propagate lanes and out of lane 15, a borrow through all 15 lanes above lane 0
    assert max(t[1] for t in top.values()) == 15 and all(t[2] == 15 for t in top.values())


def test_largest_hi_is_the_bound_of_the_derivation(table):
    """mont_mul's comment and DESIGN.md 15.16 both say `a count of at most 2`: the derivation (PO.HI_BOUND) gives 2, the model asserts it
    on every product, and the catalogue reaches it"""
    assert PO.HI_BOUND == 2 and max(t[0] for t in table[1].values()) == 2


def test_random_sweep_stays_inside_the_pinned_states(table):
    states = table[0]
    for limbs in SWEEP_LIMBS:
        for cls, c in PO.moduli(limbs, 64).items():
            rng = random.Random(0x7c00 + 64 * limbs + PO.CLASSES.index(cls))
            got = {_key(PO.mont_mul_model(rng.randrange(c), rng.getrandbits(64 * limbs), c, limbs)) for _ in range(SWEEP)}
            assert got <= states[cls], (limbs, cls, got - states[cls])


def test_searched_triples_reach_their_pinned_states():
    reached = set()
    for limbs, cls, seed, target, want in PO.SEARCHED:
        a, b, c = PO.searched_triple(limbs, cls, seed, target)
        s = PO.mont_mul_model(a, b, c, limbs)
        assert PO.searched_state(s) == want, (limbs, cls, seed, target)
        reached.add((limbs, s.out, s.res_run >= 3, s.res_run >= 3 and s.res_start + s.res_run == 16, s.sub_run >= 3))
    for limbs in (16, 32):
        assert {(limbs, 1, True, True, False), (limbs, 1, False, False, False), (limbs, 0, False, False, True)} <= reached
    assert all(any(r[0] == limbs and r[2] for r in reached) for limbs in (8, 16, 17, 32))


def test_sub_double_and_setup_models_agree_with_integers():
    """sub_model and double_mod_model assert their values themselves; setup_model asserts R mod c and R^2 mod c"""
    for limbs in PO.LIMBS_ALL:
        W = 64 * PO.GROUP * PO.capacity(limbs)
        for tb in (PO.TOP_BITS if limbs in SWEEP_LIMBS else (64,)):
            for c in PO.moduli(limbs, tb).values():
                ninv, one, r2 = PO.setup_model(c, limbs)
                assert (ninv * c + 1) % (1 << 64) == 0
                assert PO.sub_model(c, one, limbs) == PO.SubState(c - one, 0, *PO.sub_model(c, one, limbs)[2:])
                for x in PO.operands_a(c, limbs).values():
                    assert PO.sub_model(x, c, limbs).d == (x - c) % (1 << W) and PO.sub_model(x, c, limbs).borrow == 1
                    assert PO.double_mod_model(x, c, limbs).r == 2 * x % c
    # operands equal in all but one lane: the borrow crosses every equal lane above it
    for limbs in (16, 32):
        lw = 64 * PO.capacity(limbs)
        x = PO.pattern("hi32_1", limbs)
        for j in range(PO.GROUP):
            st = PO.sub_model(x, x + (1 << (lw * j)), limbs)
            assert (st.borrow, st.run, st.start) == (1, 15 - j, j + 1 if j < 15 else -1)


def test_every_structured_prime_fixture_is_a_prime_of_its_width():
    fx = PO.structured_primes()
    assert {l for l, _, _, _ in fx} == set(PO.LIMBS_ALL)
    for limbs in PO.LIMBS_ALL:
        assert {n for l, n, _, _ in fx if l == limbs} == set(PO.PATTERNS) & set(PO.moduli(limbs, 64))
    for limbs, name, k, sign in fx:
        p = PO.pattern_prime(limbs, name, k, sign)
        assert p.bit_length() == 64 * limbs and sign == (1 if name == "pow2_plus1" else -1)
        assert R.mr_first_witness(p, PO.STRUCT_BASES[13:]) == (1, 8), (limbs, name, k)      # two prime bases and the six structured ones
        # minimality where it is cheap
        if limbs <= 4:
            assert not any(R.mr_first_witness(PO.pattern_prime(limbs, name, i, sign), R.PRIME_BASES)[0] for i in range(k))


def test_proth_primes_first_reach_minus_one_where_pinned():
    fx = PO.proth_primes()
    assert [s for s, _, _ in fx] == [127, 128, 129, 1023, 1024, 1025, 1983, 1984, 1985]
    for s, k, z in fx:
        c = k * 2 ** s + 1
        assert k & 1 and c < 1 << 2048 and R.mr_first_witness(c, R.PRIME_BASES) == (1, R.ALL_PASS)
        assert PO.jacobi(z, c) == -1 and all(PO.jacobi(y, c) != -1 for y in range(2, z))
        js = [j for j in range(6) if z ** (2 ** j) < 1 << 64]
        assert 0 in js and len(js) >= 4
        for j in js:
            # base z^(2^j): c - 1 first after s - 1 - j squarings; j = 0 is bit position 1, the last the kernel's window 1 <= pos < s admits
            assert PO.first_minus_one(c, z ** (2 ** j)) == s - 1 - j
            assert R.mr_first_witness(c, (z ** (2 ** j),)) == (1, 1)


def test_small_negatives():
    assert R.mr_first_witness(341, (2,)) == (0, 0) and pow(2, 340, 341) == 1 and PO.first_minus_one(341, 2) == -1
    for c in PO.SMALL_NEGATIVES[1:]:
        assert all(pow(a, c - 1, c) == 1 for a in range(2, c) if math.gcd(a, c) == 1)
        assert R.mr_first_witness(c, R.PRIME_BASES)[0] == 0
    # a^(c-1) = -1 mod c has no solution for a composite (nor prime) odd c: literally for small c, and by the module's argument in general
    assert PO.MINUS_ONE_AT_POS_0_BELOW_2_20 == ()
    assert not any(pow(a, c - 1, c) == c - 1 for c in range(3, 512, 2) for a in range(1, c))
