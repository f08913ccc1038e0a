"""The packed ballot in the C++ host mirror (paillier_halo2_amd/host/paillier_chip.hpp: PaillierChip::pballot,
paillier_pballot_test, synthesize_pballot_circuit, pz::pballot_bases, pz::unpack_tally) driven by tests/cpp/test_pballot.cpp over the C ABI alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(force=False):
    import paillier_halo2_amd as pz

    pz.build()          # the library the program links
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "pballot.mk"] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tests", "cpp", "test_pballot")


def test_pballot_mirror_builds_and_counts():
    """CPU: the mirror with the packed ballot compiles and links against the C ABI; its cell-count checks need no device"""
    exe = _build(force=True)
    p = subprocess.run([exe, "--host-only"], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


@pytest.mark.gpu
def test_pballot_mirror_on_the_device():
    p = subprocess.run([_build()], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "ALL OK" in p.stdout
