"""GPU: the gate lines of the quotient on part A of the three-coset domain only.

The gate numerator G = sum_j y^.. q_j (a_j + a_j(wX) a_j(w^2 X) - a_j(w^3 X)) has degree <= 3n - 3 and vanishes on the whole domain, so
G / Z_H has degree <= 2n - 3: the 2n points of part A (g <w_2n>) give its coefficients without wrap-around, and only the permutation and
lookup lines need part B.  create_proof (prover.py and host/create_proof.hpp) divides the two groups apart and joins them as coefficients;
a streamed key re-extends the selectors on part A only.

  * the proof at the reference's bench shape (128-bit n, k = 14, lookup_bits 13) equals the proof over halo2's own 4n-point domain
    (cosets = 4: one part, one Horner over all lines) byte for byte, from a resident and from a streamed key;
  * the library's stepper (pz_proof_*) proves the same statement to the same verifier;
  * an unsatisfied gate, which no longer shows in the other lines' top coefficients, fails the degree check through the gate part's own
    top two coefficients;
  * pz_permutation_product_sets_dev with a short last set, chunks of 2 and of 3, against oracle/pyref.permutation_product (the kernel
    was tried with two products fewer per set and row, measured and left as it was: DESIGN.md section 6.1)."""
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests.test_gpu_connected_proof import _mont1, _verify, eng, world  # noqa: F401  (module-scoped fixtures, set up once for this file)
from tests.test_gpu_next_rows import _dev, _ints, _m

pytestmark = pytest.mark.gpu

R = P.FR_R


@pytest.mark.parametrize("m,chunk", [(5, 2), (7, 3)])
def test_permutation_product_sets_vs_oracle(eng, cref, m, chunk):
    """random canonical columns and sigma values, n = 2^6: set j starts where set j - 1 stood at row u; the last set is short in both
    shapes (one column of two, one of three), the sets before it full"""
    import torch

    k, bf = 6, 5
    n = 1 << k
    u = n - (bf + 1)
    rng = random.Random(0x7065 + m)
    w_n = P.fr_omega(k)
    delta = pow(P.FR_GENERATOR, 1 << P.FR_S, R)
    beta, gamma = rng.randrange(1, R), rng.randrange(1, R)
    val = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    sig = [[rng.randrange(R) for _ in range(n)] for _ in range(m)]
    nsets = -(-m // chunk)
    d_val, d_sig = _dev(cref, val), _dev(cref, sig)
    d_z = torch.zeros((nsets, n, 4), dtype=torch.int64, device="cuda")
    eng.permutation_product_sets_dev(d_val.data_ptr(), 4 * n, d_sig.data_ptr(), 4 * n, m, chunk, k, u, _m(cref, w_n), _m(cref, beta),
                                     _m(cref, gamma), _m(cref, delta), d_z.data_ptr(), 4 * n)
    eng.sync()
    z0 = 1
    for j in range(nsets):
        c0, mc = j * chunk, min(chunk, m - j * chunk)
        want = P.permutation_product(val[c0:c0 + mc], sig[c0:c0 + mc], w_n, beta, gamma, pow(delta, c0, R), delta, z0)
        assert _ints(cref, d_z[j]) == want, j
        z0 = want[u]


def _same(a, b):
    for f in a.commitments:
        assert np.array_equal(a.commitments[f], b.commitments[f]), f
    for f in a.evals:
        assert np.array_equal(a.evals[f], b.evals[f]), f


def _tamper(cref, st):
    j = 3
    r0 = int(np.nonzero(st.selectors[j])[0][100])

    def f(cols):
        cols[j, r0 + 3] = _mont1(cref, st.adv_cols[j][r0 + 3] + 1)      # the output cell of an enabled gate

    return f


def test_gate_lines_on_part_a_give_the_four_coset_proof(eng, cref, world):
    from paillier_halo2_amd import prover

    pk, pk4, ch, st = world["pk"], world["pk4"], world["ch"], world["st"]
    pr = prover.create_proof(pk, world["witness"](), ch, seed=11, tile=8)
    pr4 = prover.create_proof(pk4, world["witness"](), ch, seed=11, tile=8)
    assert pr.h_degree_ok and pr4.h_degree_ok
    _same(pr, pr4)
    assert _verify(cref, world, pr) == (True, True, True)
    # an unsatisfied gate fails the degree check
    bad = prover.create_proof(pk, world["witness"](), ch, seed=11, tile=8, hooks={"advice": _tamper(cref, st)})
    assert bad.h_degree_ok is False
    # a streamed key (no extended key column resident: selectors re-extended per tile, on part A only) gives the same proof ...
    pk_s = prover.keygen(eng, pk.st, pk.bases_lagrange, pk.bases_monomial, ext_resident_cols=0)
    pr_s = prover.create_proof(pk_s, world["witness"](), ch, seed=11, tile=8)
    assert pr_s.h_degree_ok
    _same(pr_s, pr4)
    # ... and the same verdict on the tampered cell
    bad_s = prover.create_proof(pk_s, world["witness"](), ch, seed=11, tile=8, hooks={"advice": _tamper(cref, st)})
    assert bad_s.h_degree_ok is False


@pytest.mark.parametrize("resident", [None, 0])
def test_stepper_proves_the_same_statement(eng, cref, world, resident):
    """the stepper draws its blinding rows from its own stream, so its proof is another proof of the same statement: it must satisfy
    the same verifier (degree, identity at x against the evaluations, openings against the commitments), and reject the tampered cell"""
    from paillier_halo2_amd import prover_native

    pk, st = world["pk"], world["st"]
    key = prover_native.NativeKey(eng, pk.st, pk.bases_lagrange, pk.bases_monomial, tile=8, ext_resident_cols=resident)
    try:
        pr = prover_native.create_proof(key, world["witness"]().data_ptr(), world["ch"], seed=11)
        assert _verify(cref, world, pr) == (True, True, True)
        cols = world["witness"]()
        _tamper(cref, st)(cols)
        bad = prover_native.create_proof(key, cols.data_ptr(), world["ch"], seed=11)
        deg, ident, opening = _verify(cref, world, bad)
        assert (deg, ident, opening) == (False, False, True)
    finally:
        key.free()
