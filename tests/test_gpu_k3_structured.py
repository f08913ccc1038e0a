"""GPU: the big-integer kernels (K3, csrc/pz_bigint.hip) against Python integers on STRUCTURED operands (tests/k3_operands.py; DESIGN.md
section 15.13): moduli that are runs of ones and zeros at limb counts just below, at and just past a team's slice boundaries, operands
that make carries ripple through every lane, propagate runs inside a number, exact zeros and maxima of quotient and remainder, every
branch of the normalisation shift, and the Barrett block of k_tally_setup read back by the team kernels.  The solo product (pz_mul_mod),
the team product over the block (pz_paillier_tally), the two-workgroup chain (pz_paillier_trace), the uniform chains (wtally, ballot,
encrypt, partial), decryption, the combiners and the inverse.  Every comparison is exact; every message names shape, modulus class and
operand class."""
import collections
import functools
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import ballot_ref as BR
from tests import decrypt_ref as DR
from tests import k3_operands as K
from tests import partial_ref as TR
from tests import shamir_ref as SR
from tests import tally_ref as TAL
from tests import wtally_ref as WR

pytestmark = pytest.mark.gpu

CASES = collections.Counter()          # entry point -> comparisons made (printed when the module's engine closes)


@pytest.fixture(scope="module")
def eng():
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    yield e
    e.close()
    print("\nk3 structured cases: " + ", ".join("%s %d" % kv for kv in sorted(CASES.items())))


def _lim(x, n):
    return np.frombuffer(x.to_bytes(8 * n, "little"), dtype=np.uint64).copy()


def _int(w):
    return int.from_bytes(np.ascontiguousarray(w, dtype=np.uint64).tobytes(), "little")


def _rows(vals, n):
    return np.stack([_lim(v, n) for v in vals])


def _recs(steps, L):
    """records (a, b, q, r) as the (len, 4, L) word array an entry point writes"""
    raw = b"".join(v.to_bytes(8 * L, "little") for st in steps for v in st)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(steps), 4, L)


def _status(fn):
    import paillier_halo2_amd as pz

    with pytest.raises(pz.PzError) as e:
        fn()
    return e.value.status


def _range():
    from paillier_halo2_amd import _lib

    return _lib.PZ_ERR_RANGE


# ------------------------------------------------------------------------------------------------- 1. the solo product, its own setup
def _mul_mod_all(eng, limbs, tb, cls, m, n=0):
    ops, mw = K.operands(m, limbs, n), _lim(m, limbs)
    for a, b in K.pairs(m, limbs, n):
        q, r = eng.mul_mod(limbs, _lim(ops[a], limbs), _lim(ops[b], limbs), mw)
        assert (_int(q), _int(r)) == divmod(ops[a] * ops[b], m), ("mul_mod", limbs, tb, cls, a, b)
        CASES["mul_mod"] += 1


@pytest.mark.parametrize("limbs,tb", K.SHAPES_M)
def test_mul_mod_equals_divmod(eng, limbs, tb):
    for cls, m in K.moduli(K.bits_of(limbs, tb)).items():
        _mul_mod_all(eng, limbs, tb, cls, m)
        un, mw = K.unreduced(m, limbs), _lim(m, limbs)
        for a, b in K.UNREDUCED_PAIRS:       # operands that need not be below m: PZ_ERR_RANGE exactly where the quotient needs more than `limbs` limbs
            q_, r_ = divmod(un[a] * un[b], m)
            call = lambda: eng.mul_mod(limbs, _lim(un[a], limbs), _lim(un[b], limbs), mw)
            if q_ >> (64 * limbs):
                assert _status(call) == _range(), ("mul_mod unreduced", limbs, tb, cls, a, b)
            else:
                q, r = call()
                assert (_int(q), _int(r)) == (q_, r_), ("mul_mod unreduced", limbs, tb, cls, a, b)
            CASES["mul_mod unreduced"] += 1


@pytest.mark.parametrize("ln,tb", [(ln, tb) for ln in (32, 64) for tb in K.TOP_BITS])
def test_mul_mod_under_the_square_of_a_full_size_n(eng, ln, tb):
    """n^2 of a 32- and a 64-limb n: the production moduli (the DPP shift at E = 1, ls = 1 beside it, ls = 0 at E = 2)"""
    for cls, n in K.moduli(K.bits_of(ln, tb)).items():
        _mul_mod_all(eng, 2 * ln, tb, cls, n * n, n)


# ------------------------------------------------------------------------------------------------- 2. the team product over a k_tally_setup block
@pytest.mark.parametrize("ln,tb", K.SHAPES_N)
def test_tally_of_two_equals_divmod(eng, ln, tb):
    L = 2 * ln
    for cls, n in K.moduli(K.bits_of(ln, tb)).items():
        m, nw = n * n, _lim(n, ln)
        ops = K.operands(m, L, n)
        for a, b in K.pairs(m, L, n):
            c, steps = eng.paillier_tally(ln, nw, _rows([ops[a], ops[b]], L))
            q, r = divmod(ops[a] * ops[b], m)
            assert tuple(_int(steps[0, j]) for j in range(4)) == (ops[a], ops[b], q, r) and _int(c) == r, ("tally", ln, tb, cls, a, b)
            CASES["tally of two"] += 1
        if m.bit_length() > 64:          # an operand equal to n^2 and one above it, in either position
            for bad, at in ((m, 0), (m + 1, 1)):
                vs = [ops["m-1"], ops["m-2"]]
                vs[at] = bad
                assert _status(lambda: eng.paillier_tally(ln, nw, _rows(vs, L))) == _range(), ("tally range", ln, tb, cls, at)
                CASES["tally range"] += 1


@pytest.mark.parametrize("count", [3, 5, 7])
@pytest.mark.parametrize("ln,tb", [(9, 33), (32, 64), (49, 1)])
def test_tally_tree_over_the_catalogue(eng, ln, tb, count):
    """the catalogue as the ciphertext list: every level, the carried odd element"""
    L = 2 * ln
    for cls, n in K.moduli(K.bits_of(ln, tb)).items():
        ops = K.operands(n * n, L, n)
        names = [k for k in ops if k != "0"]
        for off in (0, len(names) // 2, len(names) - count):
            pick = names[off:off + count]
            cts = [ops[k] for k in pick]
            root, want = TAL.tally_trace(n, cts)
            c, steps = eng.paillier_tally(ln, _lim(n, ln), _rows(cts, L))
            assert _int(c) == root and np.array_equal(steps, _recs(want, L)), ("tally tree", ln, tb, cls, pick)
            CASES["tally tree"] += 1


# ------------------------------------------------------------------------------------------------- 3. the two-workgroup chain
@pytest.mark.parametrize("tb", [1, 33, 64])
@pytest.mark.parametrize("L", [16, 18, 48, 62, 64, 66, 98, 128])
def test_trace_equals_the_reference_chain(eng, L, tb):
    for cls, m in K.moduli(K.bits_of(L, tb)).items():
        ops = K.by_name(m, L)
        hot = [k for k in ops if k.startswith("2^(64*")][-1:] or ["2^(top-1)"]
        for base in ["m-1", "alt32_hi", "alt64"] + hot:
            for e in ((1 << 12) - 1, (1 << 11) | 1, 1, 0):
                want, steps = P.pow_mod_fixed_exp_trace(ops[base], e, m)
                res, got, ns = eng.paillier_trace(L, _lim(m, L), _lim(ops[base], L), _lim(e, 1), 1)
                assert ns == len(steps) and _int(res) == want == pow(ops[base], e, m), ("trace", L, tb, cls, base, e)
                assert ns == 0 or np.array_equal(got, _recs(steps, L)), ("trace records", L, tb, cls, base, e)
                CASES["trace"] += 1


# ------------------------------------------------------------------------------------------------- 4. the uniform chains over the block
W_BITS = 6
EXPS = (0, (1 << W_BITS) - 1, 1 << (W_BITS - 1))           # zero, all ones, a single top bit


def _chain_ns(ln, tb):
    """(class, n) for the chain tests: all ones, 2^(b-1) + 1 and the 32-bit alternating modulus at the shape"""
    ms = K.moduli(K.bits_of(ln, tb))
    return [(cls, ms[cls]) for cls in ("all_ones", "pow2_plus1", "alt32_hi")]


MERSENNE_CHAIN = (3, 5)         # the 648- and the 1886-bit Mersenne n (11 and 30 limbs)
CHAIN_SHAPES = [(ln, tb) for ln in (8, 9, 31, 32, 33, 49) for tb in (1, 64, 33)] + [("mersenne", i) for i in MERSENNE_CHAIN]


def _chain_cases(ln, tb):
    if ln == "mersenne":
        p, q = K.mersenne_primes(tb)
        return K.words((p * q).bit_length()), [("mersenne%d" % K.MERSENNE_BITS[tb], p * q)]
    return ln, _chain_ns(ln, tb)


def _pick(ops, names):
    assert all(k in ops for k in names), names
    return [(k, ops[k]) for k in names]


@pytest.mark.parametrize("ln,tb", CHAIN_SHAPES)
def test_wtally_and_partial_equal_their_references(eng, ln, tb):
    ln_, cases = _chain_cases(ln, tb)
    L = 2 * ln_
    for cls, n in cases:
        ops = K.by_name(n * n, L, n)
        cts = _pick(ops, ["m-1", "alt32_hi", "1+(n-1)n"])
        vals = [v for _, v in cts]
        root, chains, tree, _, _ = WR.wtally_trace(n, vals, EXPS, W_BITS)
        c, steps = eng.paillier_wtally(ln_, _lim(n, ln_), _rows(vals, L), np.array(EXPS, dtype=np.uint64), W_BITS)
        assert _int(c) == root and np.array_equal(steps, _recs(WR.records(chains, tree), L)), ("wtally", ln, tb, cls, [k for k, _ in cts])
        CASES["wtally"] += 1
        hot = [k for k in ops if k.startswith("2^(64*")][-1:] or ["2^(top-1)"]
        pcts = _pick(ops, ["m-2", "alt64"] + hot)
        for theta in EXPS:
            tr = TR.partial_trace(n, ops["alt32_lo"], theta, [v for _, v in pcts], W_BITS)
            h, u, steps = eng.paillier_partial(ln_, _lim(n, ln_), _lim(ops["alt32_lo"], L), _lim(theta, L), _rows([v for _, v in pcts], L), W_BITS)
            assert _int(h) == tr.h and [_int(row) for row in u] == tr.us, ("partial", ln, tb, cls, theta, [k for k, _ in pcts])
            assert np.array_equal(steps, _recs(TR.records(tr), L)), ("partial records", ln, tb, cls, theta)
            CASES["partial"] += 1


def _enc_inputs(ln, tb):
    """per n of the shape: (class, n, limbs, g, [r values], where) with g and the r from the operand classes below n"""
    ln_, cases = _chain_cases(ln, tb)
    for cls, n in cases:
        ops = K.by_name(n, ln_)
        rs = _pick(ops, ["m-1", "alt32_hi", "2^(top-1)"])
        yield cls, n, ln_, ops["alt64"], [v for _, v in rs], (ln, tb, cls, [k for k, _ in rs])


@pytest.mark.parametrize("ln,tb", CHAIN_SHAPES)
def test_ballot_equals_its_reference(eng, ln, tb):
    """three messages under one key; the r^n chains run over every bit of a structured n (all ones: a product per bit)"""
    for cls, n, ln_, g, rv, where in _enc_inputs(ln, tb):
        tr = BR.ballot_trace(n, g, EXPS, rv, W_BITS)
        c, steps, nr = eng.paillier_ballot(ln_, _lim(n, ln_), _lim(g, ln_), np.array(EXPS, dtype=np.uint64), _rows(rv, ln_), W_BITS)
        assert nr == BR.n_steps_r(n) and [_int(row) for row in c] == tr.cts, ("ballot",) + where
        assert np.array_equal(steps.reshape(-1, 4, 2 * ln_), _recs(BR.records(tr), 2 * ln_)), ("ballot records",) + where
        CASES["ballot"] += 1


@pytest.mark.parametrize("ln,tb", CHAIN_SHAPES)
def test_encrypt_equals_its_reference(eng, ln, tb):
    """the exponent's own bits: m = 0 (no g chain at all), all ones, a single top bit"""
    for cls, n, ln_, g, rv, where in _enc_inputs(ln, tb):
        B = len(EXPS)
        c, steps, ng, nr = eng.paillier_encrypt(ln_, _rows([n] * B, ln_), _rows([g] * B, ln_), _rows(EXPS, ln_), _rows(rv, ln_))
        for i, (m, r) in enumerate(zip(EXPS, rv)):
            res, sg, sr, fin = P.encrypt_trace(n, g, m, r)
            want = sg + sr + [fin]
            assert (_int(c[i]), int(ng[i]), int(nr[i])) == (res, len(sg), len(sr)), ("encrypt", i) + where
            assert np.array_equal(steps[i, :len(want)], _recs(want, 2 * ln_)), ("encrypt records", i) + where
            CASES["encrypt"] += 1


@pytest.mark.parametrize("ln,tb", CHAIN_SHAPES)
def test_encrypt_uniform_equals_its_reference(eng, ln, tb):
    """W_BITS message bits in the circuit: m = 0 (the accumulator stays 1 through all 2 W_BITS records), all ones, a single top bit"""
    for cls, n, ln_, g, rv, where in _enc_inputs(ln, tb):
        B = len(EXPS)
        c, steps, ng, nr = eng.paillier_encrypt_uniform(ln_, W_BITS, _rows([n] * B, ln_), _rows([g] * B, ln_), _rows(EXPS, ln_), _rows(rv, ln_))
        for i, (m, r) in enumerate(zip(EXPS, rv)):
            res, sg, sr, fin = P.encrypt_uniform_trace(n, g, m, r, W_BITS)
            want = sg + sr + [fin]
            assert (_int(c[i]), int(ng[i]), int(nr[i])) == (res, 2 * W_BITS, len(sr)), ("encrypt_uniform", i) + where
            assert np.array_equal(steps[i, :len(want)], _recs(want, 2 * ln_)), ("encrypt_uniform records", i) + where
            CASES["encrypt_uniform"] += 1


# ------------------------------------------------------------------------------------------------- 5. decryption
KEYS = [("mersenne", i, False) for i in range(len(K.MERSENNE))] + [("structured", w, False) for w in K.STRUCTURED_KEYS]
KEYS += [("mersenne", i, True) for i in range(4)]        # a general g, found as tests/decrypt_ref.key finds it, for the four small keys


@functools.lru_cache(maxsize=None)
def _primes(kind, which):
    return K.mersenne_primes(which) if kind == "mersenne" else K.structured_key_primes(which)


def _ciphertexts(k, p, q, only=None):
    """(name, c): 1, n + 1, 1 + (n - 1) n, n^2 - 1, encryptions of 0, 1 and n - 1 under r in {1, n - 1, 2^k}, and two that are no units
    (only: the names wanted, nothing else is computed)"""
    n, g = k[0], k[1]
    out = [("1", lambda: 1), ("n+1", lambda: n + 1), ("1+(n-1)n", lambda: 1 + (n - 1) * n), ("n^2-1", lambda: n * n - 1)]
    for mn, m in (("0", 0), ("1", 1), ("n-1", n - 1)):
        for rn, r in (("1", 1), ("n-1", n - 1), ("2^k", 1 << (n.bit_length() // 2))):
            out.append(("enc(%s; %s)" % (mn, rn), lambda m=m, r=r: SR.encrypt(n, g, m, r, pq=(p, q))))
    out += [("p", lambda: p), ("p(q-2)", lambda: p * (q - 2))]
    return [(name, f()) for name, f in out if only is None or name in only]


@functools.lru_cache(maxsize=None)
def _key_cts(kind, which, only=None):
    """(key with g = n + 1, its ciphertext list): computed once, shared by the decryption and the combiner tests"""
    p, q = _primes(kind, which)
    k = K.full_key(p, q)
    return k, _ciphertexts(k, p, q, only)


@functools.lru_cache(maxsize=None)
def _plain(kind, which):
    k, cts = _key_cts(kind, which)
    return [DR.decrypt_ref(k, c) for _, c in cts]


@pytest.mark.parametrize("kind,which,general_g", KEYS)
def test_decrypt_equals_the_reference(eng, kind, which, general_g):
    p, q = _primes(kind, which)
    n = p * q
    lam = SR.lam_of(p, q)
    k = K.full_key(p, q, K.general_g(n, lam, which) if general_g else 0)
    Ln = K.words(n.bit_length())
    sk = eng.paillier_sk(Ln, *k[:4])
    try:
        assert sk.params() == (k[4], k[5]), ("sk", kind, which, general_g)
        cts = _ciphertexts(k, p, q) if general_g else _key_cts(kind, which)[1]
        m, r, flags = eng.paillier_decrypt(sk, _rows([c for _, c in cts], 2 * Ln))
        for i, (name, c) in enumerate(cts):
            assert (_int(m[i]), _int(r[i]), int(flags[i])) == DR.decrypt_ref(k, c), ("decrypt", kind, which, general_g, name)
            CASES["decrypt"] += 1
        assert _status(lambda: eng.paillier_decrypt(sk, _rows([cts[4][1], n * n], 2 * Ln))) == _range(), ("decrypt range", kind, which)
    finally:
        sk.free()


# ------------------------------------------------------------------------------------------------- 6. the combiners
COMBINE_KEYS = [("mersenne", 0), ("mersenne", 3), ("mersenne", 5), ("structured", "mixed")]
# under the 3482-bit key (E = 2) a shorter list without the non-units: the test's time is Python's own 7000-bit powers for the dealing
# and the partials (0.2 to 0.8 s each; a non-unit's cannot go through the Chinese remainder theorem).  The non-unit path runs at E = 1.
SHORT = ("1", "enc(0; n-1)", "enc(n-1; 2^k)")


@functools.lru_cache(maxsize=None)
def _dealt(kind, which, T, t):
    """(public key, shares) by keys.deal_shares (t = 0) or keys.deal_shamir with a seeded rand: once per key and scheme"""
    from paillier_halo2_amd import keys

    p, q = _primes(kind, which)
    rand = random.Random(0x6c00 + 16 * T + t).randrange
    return keys.deal_shamir(p, q, T, t, rand=rand) if t else keys.deal_shares(p, q, T, rand=rand)


@functools.lru_cache(maxsize=None)
def _partial(kind, which, T, t, i, c):
    """trustee i's (0-based) partial decryption of c, in Python integers"""
    key, shares = _dealt(kind, which, T, t)
    return SR.partial(c, shares[i], key.n, pq=_primes(kind, which))


def _check_combiner(kind, which, T, t, members, call, ref, where, only=None):
    """the decryption test's ciphertexts (plaintext 0 with every partial 1, so A = B exactly; n - 1; the two non-units), one entry whose
    first partial belongs to another ciphertext, and in a second call one entry with a partial equal to n^2: (m, flags) of every entry
    equal the reference's, and where the reference raises no flag its plaintext is decrypt_ref's.  -> the flags seen"""
    import paillier_halo2_amd as pz

    k, cts = _key_cts(kind, which, only)
    n = k[0]
    Ln = K.words(n.bit_length())
    names = [name for name, _ in cts]
    parts = [[_partial(kind, which, T, t, i, c) for _, c in cts] for i in members]
    at = names.index("enc(n-1; 2^k)")
    for row_i, row in enumerate(parts):                  # "swapped": the first partial is that of ciphertext "1", the others of enc(n - 1)
        row.append(row[names.index("1")] if row_i == 0 else row[at])
    names = names + ["swapped"]
    seen = set()

    def compare(m, flags, rows, labels):
        for j, name in enumerate(labels):
            want = ref([row[j] for row in rows])
            assert (_int(m[j]), int(flags[j])) == want, where + (name,)
            seen.add(want[1])
            if only is None and name in dict(cts):
                dm, _, dflag = _plain(kind, which)[[c[0] for c in cts].index(name)]
                assert (want == (dm, 0)) if dflag == 0 else (want[0] == 0 and want[1] != 0), where + (name, "against decrypt_ref")
            CASES[where[0]] += 1

    arr = lambda rows: np.stack([_rows(row, 2 * Ln) for row in rows])
    compare(*call(arr(parts)), parts, names)
    over = [row + [row[at]] for row in parts]
    over[-1][-1] = n * n                                  # a partial equal to n^2: PZ_ERR_RANGE, every entry written as without it
    with pytest.raises(pz.PzError) as e:
        call(arr(over))
    assert e.value.status == _range(), where + ("range",)
    compare(e.value.m, e.value.flags, over, names + ["partial = n^2"])
    assert ref([row[-1] for row in over]) == (0, 2)
    return seen


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("kind,which", COMBINE_KEYS + [("mersenne", 6)])
def test_combine_equals_the_reference(eng, kind, which, T):
    """(the 3482-bit key: k_partial_combine at E = 2, on the shorter list)"""
    key, _ = _dealt(kind, which, T, 0)
    n, Ln = key.n, K.words(key.n.bit_length())
    assert key.g == n + 1
    ref = lambda us: (0, 2) if any(u >= n * n for u in us) else TR.combine(us, n, key.mu2)
    call = lambda parts: eng.paillier_combine(Ln, _lim(n, Ln), _lim(key.mu2, Ln), parts)
    big = (kind, which) == ("mersenne", 6)
    seen = _check_combiner(kind, which, T, 0, range(T), call, ref, ("combine", kind, which, T), only=SHORT if big else None)
    assert seen == ({0, 2} if big and T == 1 else {0, 1, 2}), ("combine flags", kind, which, T, seen)


def _combine_t(eng, kind, which, T, t, ids, only=None):
    key, _ = _dealt(kind, which, T, t)
    n, Ln = key.n, K.words(key.n.bit_length())
    mus = SR.lagrange(T, ids)
    ref = lambda us: SR.combine(mus, us, n, key.mu2)
    call = lambda parts: eng.paillier_combine_t(Ln, key, ids, parts)
    return _check_combiner(kind, which, T, t, [i - 1 for i in ids], call, ref, ("combine_t", kind, which, T, t, tuple(ids)), only=only)


@pytest.mark.parametrize("T,t,ids", [(3, 2, (1, 2)), (3, 2, (3, 2)), (5, 3, (1, 2, 3)), (5, 3, (5, 4, 3))])
@pytest.mark.parametrize("kind,which", COMBINE_KEYS)
def test_combine_t_equals_the_reference(eng, kind, which, T, t, ids):
    seen = _combine_t(eng, kind, which, T, t, list(ids))
    assert {0, 1, 2, 8} <= seen, ("combine_t flags", kind, which, T, t, ids, seen)      # mismatch, a partial >= n^2, B mod n no unit


@pytest.mark.parametrize("ids", [(1, 2), (3, 2)])
def test_combine_t_under_the_3482_bit_mersenne_key(eng, ids):
    """E = 2, once: two of three trustees, on the shorter list"""
    seen = _combine_t(eng, "mersenne", 6, 3, 2, list(ids), only=SHORT)
    assert {0, 1, 2} <= seen, ("combine_t flags", "mersenne", 6, ids, seen)


# ------------------------------------------------------------------------------------------------- 7. the inverse
def _inverse_xs(m, limbs):
    bl = m.bit_length()
    ks = sorted({k for j in range(K.slice_limbs(limbs), limbs, K.slice_limbs(limbs)) for k in (64 * j - 1, 64 * j) if k < bl - 1} | {bl - 2})
    xs = [("2^%d" % k, 1 << k) for k in ks] + [("m-2^%d" % k, m - (1 << k)) for k in ks]
    xs += [("(m-1)/2", (m - 1) // 2), ("(m+1)/2", (m + 1) // 2), ("m-1", m - 1), ("m-2", m - 2), ("alt64", K.alt64(bl - 1)),
           ("alt32_hi", K.alt32_hi(bl - 1)), ("alt32_lo", K.alt32_lo(bl - 1)), ("0", 0), ("1", 1)]
    return xs


def _check_inverse(eng, limbs, m, xs, where):
    inv, flags = eng.mod_inverse(limbs, _lim(m, limbs), _rows([x for _, x in xs], limbs))
    for j, (name, x) in enumerate(xs):
        assert (_int(inv[j]), int(flags[j])) == SR.inverse(x, m), ("mod_inverse",) + where + (name,)
        CASES["mod_inverse"] += 1


@pytest.mark.parametrize("tb", [1, 33, 64])
@pytest.mark.parametrize("limbs", [16, 18, 62, 64, 66, 98, 128])
def test_inverse_equals_pow(eng, limbs, tb):
    for cls, m in K.odd_only(K.moduli(K.bits_of(limbs, tb))).items():
        _check_inverse(eng, limbs, m, _inverse_xs(m, limbs), (limbs, tb, cls))


@pytest.mark.parametrize("i", [4, 5, 6])
def test_inverse_under_a_mersenne_n(eng, i):
    """p and a multiple of q are no units; n of 18, 30 and 55 limbs, and n^2 of the 30-limb one (60 limbs)"""
    p, q = K.mersenne_primes(i)
    n = p * q
    for m in (n, n * n) if i == 5 else (n,):
        limbs = K.words(m.bit_length())
        xs = _inverse_xs(m, limbs) + [("p", p), ("3q", 3 * q), ("n-p", n - p)]
        assert [SR.inverse(x, m)[1] for _, x in xs[-3:]] == [1, 1, 1]
        _check_inverse(eng, limbs, m, xs, ("mersenne", K.MERSENNE_BITS[i], m == n))
