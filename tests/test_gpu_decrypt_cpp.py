"""Decryption in the C++ host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierSecretKey, PaillierChip::decrypt,
paillier_decrypt_test) driven by tests/cpp/test_decrypt.cpp on keys and ciphertexts from tests/decrypt_ref.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(force=False):
    from oracle import cref

    cref.build()        # the C oracle the program links
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "decrypt.mk"] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "cpp", "test_decrypt")


def test_decrypt_mirror_builds():
    """CPU: the mirror with decryption compiles and links against the C ABI"""
    assert os.path.exists(_build(force=True))


@pytest.mark.gpu
def test_decrypt_mirror_on_the_device(tmp_path):
    from tests import decrypt_ref as DR

    lines = []
    for bits, standard_g in ((128, False), (264, True), (2112, False)):
        k = DR.key(bits, standard_g)
        ms, _, cs = DR.encryptions(k, 3, 0xdec8 + bits)
        p, _ = DR.primes(bits)
        pairs = list(zip(cs, ms)) + [(p * 0x10001, 0)]          # the last one is no unit
        lines += ["%x" % v for v in k[:4]] + ["%x" % len(pairs)] + ["%x" % v for pair in pairs for v in pair]
    path = tmp_path / "decrypt_inputs.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([_build(), str(path)], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ALL OK" in p.stdout
