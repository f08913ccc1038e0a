"""t-of-T threshold decryption in the C++ host mirror (paillier_halo2_amd/host/paillier_chip.hpp: deal_shamir,
PaillierChip::combine_t / mod_inverse) driven by tests/cpp/test_shamir.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(force=False):
    import paillier_halo2_amd as pz

    pz.build()          # the HIP library the program links
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "shamir.mk"] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "cpp", "test_shamir")


def test_shamir_mirror_builds():
    """CPU: the mirror with the t-of-T threshold decryption compiles and links against the C ABI"""
    assert os.path.exists(_build(force=True))


@pytest.mark.gpu
def test_shamir_mirror_on_the_device():
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ALL OK" in p.stdout
