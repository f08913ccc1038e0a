"""GPU: the permutation and lookup lines of the quotient on part A of the three-coset domain only (the algebra in
Python integers: tests/test_two_coset_algebra.py).

Kernels, at k = 6, bf = 5 on random inputs (which satisfy nothing: every line is non-zero everywhere):
  * the split forms of both line kernels against the unsplit ones on a 2n-point domain, in several set-range calls, m = 5 and 7 with chunks
    of 2 and 3 (a short last set) and m = 2 (one set: no chaining lines), three lookups: Low + l_active * D equals the unsplit accumulator;
  * pz_quotient_d_rows_dev against Python integers for the same shapes, the wrap of row n - 1 to z(w^0) included;
  * pz_fr_mul_row_dev.
Proofs, at the reference's bench shape (128-bit n, k = 14, tile 8):
  * the proof equals the proof over halo2's own 4n-point domain (cosets = 4) byte for byte, from a resident and from a streamed key;
  * the library's stepper (pz_proof_*) proves the same statement to the same verifier;
  * a permutation product, or a lookup product, altered on an active row fails the degree check (through D_2's top coefficients: such a
    product leaves every line outside D as it was, except the boundary rows the alteration does not touch)."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests.test_gpu_connected_proof import _mont1, _verify, eng, world  # noqa: F401  (module-scoped fixtures, set up once for this file)
from tests.test_gpu_next_rows import _dev, _ints, _m

pytestmark = pytest.mark.gpu

R = P.FR_R
K, BF = 6, 5
N = 1 << K
U = N - (BF + 1)
DELTA = pow(P.FR_GENERATOR, 1 << P.FR_S, R)
SHAPES = [(5, 2), (7, 3), (2, 2)]
LK = 3


def _rand(rng, rows, cols):
    return [[rng.randrange(R) for _ in range(cols)] for _ in range(rows)]


@pytest.mark.parametrize("m,chunk", SHAPES)
def test_split_lines_sum_to_the_unsplit_ones(eng, cref, m, chunk):
    rng = random.Random(0x2c0 + m)
    log_ext, rot = K + 1, 2
    Ne = 1 << log_ext
    S = -(-m // chunk)
    cg, w_ext = pow(P.FR_GENERATOR, (R - 1) // 3, R), P.fr_omega(log_ext)
    beta, gamma, y = (rng.randrange(1, R) for _ in range(3))
    F = lambda v: _m(cref, v)
    cols, sig, z = (_dev(cref, _rand(rng, c, Ne)) for c in (m, m, S))
    lrows = _rand(rng, 3, Ne)
    l_ = _dev(cref, lrows)
    a, ap, sp, zl = (_dev(cref, _rand(rng, LK, Ne)) for _ in range(4))
    table = _dev(cref, _rand(rng, 1, Ne))
    h0, d0 = _rand(rng, 1, Ne)[0], _rand(rng, 1, Ne)[0]
    # the unsplit accumulator starts from h0 + l_active d0, the split ones from h0 and d0
    un = _dev(cref, [(h + la * d) % R for h, la, d in zip(h0, lrows[2], d0)])
    low, dd = _dev(cref, h0), _dev(cref, d0)
    ranges = [(0, 2), (2, 1)] if S == 3 else [(0, 1)]
    assert sum(ns for _, ns in ranges) == S
    for set_lo, ns in ranges:
        c0 = set_lo * chunk
        cnt = min(m - c0, ns * chunk)
        common = (cols[c0].data_ptr(), 4 * Ne, sig[c0].data_ptr(), 4 * Ne, z.data_ptr(), 4 * Ne, S, set_lo, ns, chunk, cnt, set_lo == 0,
                  log_ext, rot, BF + 1, l_[0].data_ptr(), l_[1].data_ptr())
        chal = (F(beta), F(gamma), F(DELTA), F(cg), F(w_ext), F(y))
        eng.quotient_permutation_part_dev(*common, l_[2].data_ptr(), *chal, un.data_ptr())
        eng.quotient_permutation_split_dev(*common, *chal, low.data_ptr(), dd.data_ptr())
    eng.sync()

    def check(what):
        got_un, got_low, got_d = _ints(cref, un), _ints(cref, low), _ints(cref, dd)
        assert any(got_d) and any(got_low)
        assert [(lo + la * d) % R for lo, la, d in zip(got_low, lrows[2], got_d)] == got_un, what

    check("permutation")
    lk = (a.data_ptr(), 4 * Ne, table.data_ptr(), ap.data_ptr(), 4 * Ne, sp.data_ptr(), 4 * Ne, zl.data_ptr(), 4 * Ne, LK, log_ext, rot,
          l_[0].data_ptr(), l_[1].data_ptr(), l_[2].data_ptr(), F(beta), F(gamma), F(y))
    eng.quotient_lookup_dev(*lk, un.data_ptr())
    eng.quotient_lookup_split_dev(*lk, low.data_ptr(), dd.data_ptr())
    eng.sync()
    check("lookup")


@pytest.mark.parametrize("m,chunk", SHAPES)
def test_d_rows_vs_python_integers(eng, cref, m, chunk):
    import torch

    rng = random.Random(0xd10 + m)
    S = -(-m // chunk)
    w = P.fr_omega(K)
    beta, gamma, y = (rng.randrange(1, R) for _ in range(3))
    F = lambda v: _m(cref, v)
    cols, sig, z = _rand(rng, m, N), _rand(rng, m, N), _rand(rng, S, N)
    a, ap, sp, zl = (_rand(rng, LK, N) for _ in range(4))
    table = _rand(rng, 1, N)[0]
    want = [0] * N
    for i in range(U, N):
        nx = (i + 1) % N                                  # row n - 1 reads z(w^0)
        acc = 0
        for j in range(S):
            left, right = z[j][nx], z[j][i]
            for c in range(j * chunk, min(m, (j + 1) * chunk)):
                left = left * (cols[c][i] + beta * sig[c][i] + gamma) % R
                right = right * (cols[c][i] + beta * pow(DELTA, c, R) * pow(w, i, R) + gamma) % R
            acc += (left - right) * pow(y, (S - 1 - j) + 5 * LK, R)
        for l in range(LK):
            d = zl[l][nx] * (ap[l][i] + beta) * (sp[l][i] + gamma) - zl[l][i] * (a[l][i] + beta) * (table[i] + gamma)
            acc += d * pow(y, 5 * (LK - 1 - l) + 2, R)
        want[i] = acc % R
    d_ = [_dev(cref, t) for t in (cols, sig, z, a, [table], ap, sp, zl)]
    out = torch.full((N, 4), -1, dtype=torch.int64, device="cuda")     # the rows below u must be WRITTEN as zero
    eng.quotient_d_rows_dev(d_[0].data_ptr(), 4 * N, d_[1].data_ptr(), 4 * N, d_[2].data_ptr(), 4 * N, m, chunk, d_[3].data_ptr(), 4 * N,
                            d_[4].data_ptr(), d_[5].data_ptr(), 4 * N, d_[6].data_ptr(), 4 * N, d_[7].data_ptr(), 4 * N, LK, K, U, F(w), F(beta),
                            F(gamma), F(DELTA), F(y), out.data_ptr())
    eng.sync()
    assert _ints(cref, out) == want and all(want[U:])


def test_fr_mul_row(eng, cref):
    rng = random.Random(0x309)
    n = 300                                               # more than one workgroup, not a multiple of it
    a, row = _rand(rng, 2, n), _rand(rng, 1, n)[0]
    d_a, d_row = _dev(cref, a), _dev(cref, row)
    eng.fr_mul_row_dev(d_a.data_ptr(), 2, 4 * n, n, d_row.data_ptr(), d_a.data_ptr(), 4 * n)       # in place
    eng.sync()
    assert _ints(cref, d_a) == [x * r % R for col in a for x, r in zip(col, row)]


def _same(a, b):
    for f in a.commitments:
        assert np.array_equal(a.commitments[f], b.commitments[f]), f
    for f in a.evals:
        assert np.array_equal(a.evals[f], b.evals[f]), f


def test_lines_on_part_a_give_the_four_coset_proof(eng, cref, world):
    from paillier_halo2_amd import prover

    pk, pk4, ch = world["pk"], world["pk4"], world["ch"]
    pr = prover.create_proof(pk, world["witness"](), ch, seed=13, tile=8)
    pr4 = prover.create_proof(pk4, world["witness"](), ch, seed=13, tile=8)
    assert pr.h_degree_ok and pr4.h_degree_ok
    _same(pr, pr4)
    assert _verify(cref, world, pr) == (True, True, True)
    # a streamed key (no extended key column resident: sigma re-extended per tile, on part A only) gives the same proof
    pk_s = prover.keygen(eng, pk.st, pk.bases_lagrange, pk.bases_monomial, ext_resident_cols=0)
    pr_s = prover.create_proof(pk_s, world["witness"](), ch, seed=13, tile=8)
    assert pr_s.h_degree_ok
    _same(pr_s, pr4)


@pytest.mark.parametrize("resident", [None, 0])
def test_stepper_proof_verifies(eng, cref, world, resident):
    from paillier_halo2_amd import prover_native

    pk = world["pk"]
    key = prover_native.NativeKey(eng, pk.st, pk.bases_lagrange, pk.bases_monomial, tile=8, ext_resident_cols=resident)
    try:
        pr = prover_native.create_proof(key, world["witness"]().data_ptr(), world["ch"], seed=13)
        assert _verify(cref, world, pr) == (True, True, True)
    finally:
        key.free()


@pytest.mark.parametrize("which", ["permutation", "lookup"])
def test_product_altered_on_an_active_row_fails_the_degree_check(eng, cref, world, which):
    from paillier_halo2_amd import prover

    def alter(Z, Zl):
        t = Z if which == "permutation" else Zl
        t[1, 1000] = _mont1(cref, 0x5eed)                 # row 1000 of 2^14: active

    bad = prover.create_proof(world["pk"], world["witness"](), world["ch"], seed=13, tile=8, hooks={"products": alter})
    assert bad.h_degree_ok is False
