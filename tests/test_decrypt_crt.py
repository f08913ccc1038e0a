"""CPU: decryption by the CRT as tests/decrypt_crt_ref.py restates it, against tests/decrypt_ref.py's textbook
form in Python integers; what the catalogue of structured ciphertexts holds; and that the host mirror's test program builds."""
import os
import subprocess

import pytest

from tests import decrypt_crt_ref as CR
from tests import decrypt_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bits", DR.KEY_BITS)
@pytest.mark.parametrize("standard_g", [True, False], ids=["g=n+1", "general-g"])
def test_crt_reference_equals_the_textbook_form(bits, standard_g):
    k = CR.key(bits, standard_g)
    n = k[0]
    for label, c, m, r in CR.catalogue(bits, standard_g):
        got = CR.decrypt_crt_ref(CR.crt_key(bits, standard_g), c)
        assert got == CR.decrypt_crt_ref(CR.crt_key(bits, standard_g, True), c), (label, "swapped primes")
        if c >= n * n:
            assert got == (0, 0, CR.FLAG_RANGE), label
            continue
        assert got == DR.decrypt_ref(k, c), label
        assert got == (m, r, int(label in CR.NON_UNITS)), label


@pytest.mark.parametrize("bits", DR.KEY_BITS)
def test_catalogue_borrows_both_ways_and_not_at_all(bits):
    """Garner's difference of the plaintexts is negative, positive and zero within every key's catalogue (and of the randomness both
    ways too)"""
    p, q = DR.primes(bits)
    n = p * q
    cat = CR.catalogue(bits, False)
    entries = [e for e in cat if e[0] not in CR.NON_UNITS and e[1] < n * n]
    assert {CR.garner_sign(p, q, m) for _, _, m, _ in entries} == {-1, 0, 1}
    assert {CR.garner_sign(p, q, r) for _, _, _, r in entries} >= {-1, 1}
    by = {label: m for label, _, m, _ in entries}
    assert by["m<min(p,q)"] % p == by["m<min(p,q)"] % q and CR.garner_sign(p, q, by["m<min(p,q)"]) == 0
    assert CR.garner_sign(p, q, by["m_p<m_q"]) == -1 and CR.garner_sign(p, q, by["m_p>m_q"]) == 1
    assert [e[0] for e in cat] == ["m=0", "m=1", "m=n-1", "m=p", "m=q", "m<min(p,q)", "m_p<m_q", "m_p>m_q", "r=1", "r+n", "p*k", "q", "0",
                                   "n^2-1", "n^2"]


def test_fixtures_order_their_primes_both_ways():
    """swapped primes are accepted: the fixtures themselves hold a key with p > q and one with p < q"""
    p, q = DR.primes(128)
    assert p > q
    p, q = DR.primes(264)
    assert p < q
    # and every fixture key passes the handle's acceptance rule: p^2 and q^2 fit the words of n
    for bits in DR.KEY_BITS:
        words = -(-bits // 64)
        assert all((v * v).bit_length() <= 64 * words for v in DR.primes(bits)), bits


def test_decrypt_crt_mirror_builds():
    """the mirror with CRT decryption compiles and links against the C ABI"""
    from oracle import cref

    cref.build()        # the C oracle the program links
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "decrypt_crt.mk", "-B"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_decrypt_crt"))
