"""The weighted tally in the C++ host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::mul_scalar / weighted_tally,
paillier_wtally_test) driven by tests/cpp/test_wtally.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(force=False):
    from oracle import cref

    cref.build()        # the C oracle the program links
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "wtally.mk"] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "cpp", "test_wtally")


def test_wtally_mirror_builds():
    """CPU: the mirror with the weighted tally compiles and links against the C ABI"""
    assert os.path.exists(_build(force=True))


@pytest.mark.gpu
def test_wtally_mirror_on_the_device():
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ALL OK" in p.stdout
