"""The ballot in the C++ host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::ballot, paillier_ballot_test,
synthesize_ballot_circuit) driven by tests/cpp/test_ballot.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(force=False):
    from oracle import cref

    cref.build()        # the C oracle the program links
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "ballot.mk"] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "cpp", "test_ballot")


def test_ballot_mirror_builds():
    """CPU: the mirror with the ballot compiles and links against the C ABI"""
    assert os.path.exists(_build(force=True))


@pytest.mark.gpu
def test_ballot_mirror_on_the_device():
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ALL OK" in p.stdout
