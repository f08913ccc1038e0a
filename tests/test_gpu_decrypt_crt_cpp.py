"""CRT decryption in the C++ host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierSecretKey::create_crt, PaillierChip::decrypt's
CrtPath, paillier_decrypt_crt_test) driven by tests/cpp/test_decrypt_crt.cpp on keys and ciphertexts from
tests/decrypt_ref.py: the CRT path = the lambda path = expected, one non-unit included."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    from oracle import cref

    cref.build()        # the C oracle the program links
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "decrypt_crt.mk"], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "cpp", "test_decrypt_crt")


@pytest.mark.gpu
def test_decrypt_crt_mirror_on_the_device(tmp_path):
    from tests import decrypt_ref as DR

    lines = []
    for bits, standard_g in ((128, False), (264, True), (2112, False)):
        k = DR.key(bits, standard_g)
        ms, _, cs = DR.encryptions(k, 3, 0xdec9 + bits)
        p, q = DR.primes(bits)
        pairs = list(zip(cs, ms)) + [(p * 0x10001, 0)]          # the last one is no unit
        lines += ["%x" % v for v in k[:4] + (p, q)] + ["%x" % len(pairs)] + ["%x" % v for pair in pairs for v in pair]
    path = tmp_path / "decrypt_crt_inputs.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([_build(), str(path)], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ALL OK" in p.stdout
