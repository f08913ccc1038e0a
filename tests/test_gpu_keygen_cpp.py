"""Prime generation in the C++ host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::is_probable_prime / prime_search,
generate_prime, generate_key, primes_are_safe) driven by tests/cpp/test_keygen.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(force=False):
    import paillier_halo2_amd as pz

    pz.build()          # the HIP library the program links
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "keygen.mk"] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "cpp", "test_keygen")


def test_keygen_mirror_builds():
    """CPU: the mirror with the prime generation compiles and links against the C ABI"""
    assert os.path.exists(_build(force=True))


@pytest.mark.gpu
def test_keygen_mirror_on_the_device():
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ALL OK" in p.stdout
