"""CPU: decryption's restatement and the decrypt circuit (kind 5 / "decrypt") -- the reference round trip over
every fixture key, kind 5 against kind 2 (the same cells, another statement), the statement's layout, the keys helper.  No device."""
import ctypes as C
import math
import random

import numpy as np
import pytest

from oracle import pyref as P
from tests import decrypt_ref as DR

UNI = dict(bits=128, W=64, lb=14, k=15)        # tests/public_ref.py's uniform shape


@pytest.mark.parametrize("bits", DR.KEY_BITS)
@pytest.mark.parametrize("standard_g", [True, False], ids=["g=n+1", "general-g"])
def test_decrypt_ref_round_trips_the_oracle_encryption(bits, standard_g):
    k = DR.key(bits, standard_g)
    n, g, lam, d, mu, ginv = k
    assert n.bit_length() == bits and g < (1 << (64 * -(-bits // 64))) and n * d % lam == 1 and g * ginv % n == 1
    count = 4 if bits <= 2112 else 2        # (Python's own modular powers at 3072 and 4096 bits take a second each)
    ms, rs, cs = DR.encryptions(k, count, 0xdec0 + bits)
    assert ms[:3] == [0, 1, n - 1][:count]
    for m, r, c in zip(ms, rs, cs):
        assert DR.decrypt_ref(k, c) == (m, r, 0)
        assert P.paillier_enc_native(n, g, m, r) == c          # also for the one made with r + n
    p, _ = DR.primes(bits)
    assert DR.decrypt_ref(k, p * 12345) == (0, 0, 1)


def test_kind5_cell_counts_equal_kind2():
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import layout

    L = pz._lib.lib()
    for bits, W, lb in ((128, 64, 14), (128, 64, 10), (264, 88, 11)):
        Ln = bits // W
        ng = 2 * Ln * W
        for nr in (0, 7, 200):
            got = []
            for kind in (2, 5):
                a, l = C.c_size_t(), C.c_size_t()
                assert L.pz_circuit_cells(kind, Ln, W, lb, ng, nr, C.byref(a), C.byref(l)) == 0
                got.append((a.value, l.value))
            cc = layout.circuit_cells("decrypt", Ln, W, lb, ng, nr)
            cu = layout.circuit_cells("encrypt_uniform", Ln, W, lb, ng, nr)
            assert got[0] == got[1] == (cc.advice, cc.lookup) == (cu.advice, cu.lookup) and cc.seg == cu.seg
        a = C.c_size_t()
        assert L.pz_circuit_cells(5, Ln, W, lb, ng + 2, 0, C.byref(a), None) == pz._lib.PZ_ERR_INVALID
        assert L.pz_circuit_cells(6, Ln, W, lb, ng, 0, C.byref(a), None) == pz._lib.PZ_ERR_INVALID


def test_structure_arrays_equal_kind2_but_for_the_exposed_list():
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import circuit_structure as CS

    bits, W, lb = UNI["bits"], UNI["W"], UNI["lb"]
    Ln = bits // W
    n, g, m, r = P.synth_paillier_inputs(bits, 0x51, standard_g=False)
    c = P.paillier_enc_native(n, g, m, r)
    sd = CS.stream_structure("decrypt", bits, W, lb, 0, n)
    su = CS.stream_structure("encrypt_uniform", bits, W, lb, 0, n)
    for f in ("n_cells", "constants", "result_cell", "n_steps_g", "n_steps_r"):
        assert getattr(sd, f) == getattr(su, f), f
    for f in ("src", "gate_mask", "lookup_src"):
        assert np.array_equal(getattr(sd, f), getattr(su, f)), f
    want, adv = DR.exposed_cells(n, g, m, r, c, bits, W, lb)
    assert sd.public_cells.tolist() == want and len(want) == 5 * Ln
    assert su.public_cells.tolist() == want[:2 * Ln] + want[3 * Ln:]
    assert [adv[i] for i in want] == DR.statement(n, g, m, c, bits, W)
    # pz_circuit_public_cells: host logic inside the library
    L = pz._lib.lib()
    out, npub = np.zeros(5 * Ln, dtype=np.uint64), C.c_size_t()
    assert L.pz_circuit_public_cells(5, Ln, W, lb, sd.n_steps_g, sd.n_steps_r, out.ctypes.data, 5 * Ln, C.byref(npub)) == 0
    assert npub.value == 5 * Ln and out.tolist() == want
    assert L.pz_circuit_public_cells(5, Ln, W, lb, sd.n_steps_g, sd.n_steps_r, None, 0, C.byref(npub)) == 0 and npub.value == 5 * Ln
    assert L.pz_circuit_public_cells(2, Ln, W, lb, sd.n_steps_g, sd.n_steps_r, None, 0, C.byref(npub)) == 0 and npub.value == 4 * Ln


def test_public_inputs_layout_and_the_range_of_m():
    from paillier_halo2_amd import verifier as PV

    bits, W = 264, 88
    k = DR.key(bits, standard_g=False)
    n, g = k[0], k[1]
    ms, rs, cs = DR.encryptions(k, 4, 0xdec1)
    for m, c in zip(ms, cs):
        st = PV.public_inputs("decrypt", n, g, c, m=m, enc_bits=bits, limb_bits=W)
        assert st == DR.statement(n, g, m, c, bits, W) and len(st) == 5 * (bits // W)
    kw = dict(enc_bits=bits, limb_bits=W)
    for bad_m in (n, n + 1, -1):
        with pytest.raises(ValueError):
            PV.public_inputs("decrypt", n, g, cs[0], m=bad_m, **kw)
    with pytest.raises(ValueError):
        PV.public_inputs("decrypt", n, g, cs[0], **kw)                   # no m
    with pytest.raises(ValueError):
        PV.public_inputs("encrypt_uniform", n, g, cs[0], m=ms[0], **kw)  # m belongs to the decrypt statement
    with pytest.raises(ValueError):
        PV.public_inputs("decrypt", n, g, 1 << (2 * bits), m=ms[0], **kw)  # c does not fit


def test_keys_helper():
    from paillier_halo2_amd import keys

    for bits in (128, 264, 2048):
        p, q = DR.primes(bits)
        n, g, lam, d, mu, ginv = DR.key(bits)
        assert keys.secret_from_primes(p, q) == (n, n + 1, lam, d)
        ng, gg = DR.key(bits, standard_g=False)[:2]
        assert keys.secret_from_primes(p, q, gg) == (n, gg, lam, d) and lam == math.lcm(p - 1, q - 1)
        with pytest.raises(ValueError):
            keys.secret_from_primes(p, q, 1)                 # order 1
        with pytest.raises(ValueError):
            keys.secret_from_primes(p, q, p)                 # no unit
    with pytest.raises(ValueError):
        keys.secret_from_primes(7, 7)
    with pytest.raises(ValueError):
        keys.secret_from_primes(3, 7)                        # gcd(21, 12) = 3
    rng = random.Random(5)
    n, g, lam, d = keys.secret_from_primes(11, 17)
    m, r = rng.randrange(n), 2
    c = P.paillier_enc_native(n, g, m, r)
    u = pow(c, lam, n * n)
    assert (u // n) * pow(pow(g, lam, n * n) // n, -1, n) % n == m and pow(c % n * pow(pow(g, -1, n), m, n) % n, d, n) == r
