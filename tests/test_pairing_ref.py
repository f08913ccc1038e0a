"""CPU: the Python restatement of the BN254 pairing (tests/bn254_pairing_ref.py) is a pairing, and the constants the HIP pairing is
compiled with (csrc/fp12_gen.cuh, made by csrc/gen_fp12.py) are the restatement's."""
import os
import random
import re
import subprocess
import sys

import pytest

from tests import bn254_pairing_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paillier_halo2_amd", "csrc")


def test_bn_parameters():
    x = B.X
    assert B.P == 21888242871839275222246405745257275088696311157297823662689037894645226208583
    assert B.R == 21888242871839275222246405745257275088548364400416034343698204186575808495617
    assert B.P == 36 * x**4 + 36 * x**3 + 24 * x**2 + 6 * x + 1 and B.R == 36 * x**4 + 36 * x**3 + 18 * x**2 + 6 * x + 1
    assert (B.P**4 - B.P**2 + 1) % B.R == 0
    assert B.ATE == 29793968203157093288 and B.HARD.bit_length() == 761
    assert B.FINAL == (B.P**6 - 1) * (B.P**2 + 1) * B.HARD


def test_g2_generator_on_twist_with_order_r():
    assert B.g2_on_curve(B.G2)
    assert B.g2_mul(B.G2, B.R, reduce=False) is None
    assert B.g2_mul(B.G2, B.R - 1) == B.g2_neg(B.G2)
    # pi(Q) = [p] Q on G2 (the Frobenius constants of the twist)
    assert B.g2_frob(B.G2) == B.g2_mul(B.G2, B.P)


def test_tower_identities():
    rng = random.Random(3)
    a = B.f12_from_coeffs([(rng.randrange(B.P), rng.randrange(B.P)) for _ in range(6)])
    assert B.f12_mul(a, B.f12_inv(a)) == B.F12_ONE
    assert B.f12_frob(a, 1) == B.f12_pow(a, B.P)
    assert B.f12_frob(a, 2) == B.f12_frob(B.f12_frob(a, 1), 1)
    assert B.f12_frob(a, 3) == B.f12_frob(B.f12_frob(a, 2), 1)
    assert B.f12_frob(a, 6) == B.f12_conj(a)


def test_pairing_bilinear_nondegenerate_order_r():
    rng = random.Random(7)
    e = B.pairing(B.G1, B.G2)
    assert e != B.F12_ONE
    assert B.f12_pow(e, B.R) == B.F12_ONE
    a, b = rng.randrange(1, B.R), rng.randrange(1, B.R)
    pa, qb = B.g1_mul(B.G1, a), B.g2_mul(B.G2, b)
    eab = B.f12_pow(e, a * b % B.R)
    assert B.pairing(pa, qb) == eab
    assert B.pairing(B.g1_mul(B.G1, a * b), B.G2) == eab
    # the shortcut final exponentiation is exactly the plain one
    f = B.miller_loop([(pa, qb)])
    assert B.final_exp(f) == B.final_exp_plain(f)
    # identities contribute 1; a product check holds exactly when built to
    assert B.pairing(None, B.G2) == B.F12_ONE and B.pairing(B.G1, None) == B.F12_ONE
    assert B.pairing_check([(B.g1_mul(B.G1, a * b), B.G2), (B.g1_neg(pa), qb)]) == 1
    assert B.pairing_check([(B.g1_mul(B.G1, a * b + 1), B.G2), (B.g1_neg(pa), qb)]) == 0
    assert B.pairing_check([((1, 3), B.G2)]) == -1


def _parse_u32_array(text, name):
    m = re.search(r"%s\[\d+\] = \{(.*?)\};" % name, text, flags=re.S)
    return [int(v[:-1], 16) for v in re.findall(r"0x[0-9a-f]+u", m.group(1))]


def _fq_from_limbs(ls):
    v = sum(l << (32 * i) for i, l in enumerate(ls))
    assert v < B.P
    return v * pow(B.MONT, -1, B.P) % B.P


def test_generated_constants_match_the_restatement():
    text = open(os.path.join(CSRC, "fp12_gen.cuh")).read()
    # the committed header is what the generator prints
    out = subprocess.run([sys.executable, os.path.join(CSRC, "gen_fp12.py")], capture_output=True, text=True, check=True).stdout
    assert out.strip() == text.strip()
    frob = _parse_u32_array(text, "PZ_FROB")
    assert len(frob) == 240
    for k in (1, 2, 3):
        want = B.frob_consts(k)
        for e in range(1, 6):
            o = ((k - 1) * 5 + (e - 1)) * 16
            assert (_fq_from_limbs(frob[o:o + 8]), _fq_from_limbs(frob[o + 8:o + 16])) == want[e], (k, e)
    tb = _parse_u32_array(text, "PZ_TWIST_B")
    assert (_fq_from_limbs(tb[:8]), _fq_from_limbs(tb[8:])) == B.B2
    assert _fq_from_limbs(_parse_u32_array(text, "PZ_TWO_INV")) == pow(2, -1, B.P)
    ate = _parse_u32_array(text, "PZ_ATE")
    assert sum(v << (32 * i) for i, v in enumerate(ate)) == B.ATE
    assert int(re.search(r"#define PZ_ATE_BITS (\d+)", text).group(1)) == B.ATE.bit_length()
    hard = _parse_u32_array(text, "PZ_HARD")
    assert sum(v << (32 * i) for i, v in enumerate(hard)) == B.HARD
    assert int(re.search(r"#define PZ_HARD_BITS (\d+)", text).group(1)) == 761
    m = re.search(r"PZ_G2_GEN\[16\] = \{(.*?)\};", text, flags=re.S)
    words = [int(v[:-3], 16) for v in re.findall(r"0x[0-9a-f]+ull", m.group(1))]
    assert B.g2_from_words(words) == B.G2 and words == B.g2_words(B.G2)


def test_g2_generator_entry_point_matches():
    """pz_g2_generator is host code: no GPU needed"""
    import numpy as np

    import paillier_halo2_amd as pz

    out = np.zeros(16, dtype=np.uint64)
    assert pz.lib().pz_g2_generator(out.ctypes.data) == 0
    assert B.g2_from_words(out) == B.G2


def test_zero_g2_params_rejected_without_gpu(tmp_path):
    """a params file whose G2 elements are zero cannot back a verifier: ValueError, before any device work"""
    import numpy as np

    from paillier_halo2_amd import srs, verifier

    k = 2
    pts = np.zeros((1 << k, 8), dtype=np.uint64)
    path = str(tmp_path / "p.srs")
    srs.write_params_kzg(path, k, pts, pts)
    params = srs.read_params_kzg(path)
    with pytest.raises(ValueError):
        verifier.VerifierParams.from_params(params)
