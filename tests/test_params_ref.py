"""CPU: the references of the params-file tests hold on their own -- the Fq2 square root and the 64-byte G2 codec (tests/g2_wire_ref.py), the
twist points outside the order-r subgroup, the Python SRS and its three file formats (tests/params_ref.py) -- and what of the new surface
needs no GPU: pz_params_file_bytes, the entry points' NULL-context refusals, and the compiled driver host/params_tool.cpp, which builds
against the C ABI alone and refuses bad input before it touches a device."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import bn254_pairing_ref as B
from tests import g2_wire_ref as G2W
from tests import params_ref as PR
from tests import wire_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pz_g2_compress", "pz_g2_decompress", "pz_g2_check_dev", "pz_g2_check", "pz_params_file_bytes", "pz_params_decode", "pz_params_from_dev",
       "pz_params_info", "pz_params_points", "pz_params_bases", "pz_params_encode", "pz_params_downsize", "pz_params_check", "pz_params_free")


def test_f2_sqrt_against_f2_sqr():
    rng = random.Random(3)
    roots = 0
    for _ in range(40):
        a = (rng.randrange(B.P), rng.randrange(B.P))
        sq = B.f2_sqr(a)
        r = G2W.f2_sqrt(sq)
        assert r is not None and B.f2_sqr(r) == sq and r in (a, B.f2_neg(a))
        r = G2W.f2_sqrt(a)
        roots += r is not None
        assert r is None or B.f2_sqr(r) == a
        # a non-square times a square stays a non-square
        assert (G2W.f2_sqrt(B.f2_mul(a, sq)) is None) == (r is None)
    assert 8 < roots < 32                                   # about half of Fq2 are squares
    # a1 = 0: squares and non-squares of Fq both have roots in Fq2
    for a0 in (0, 1, 4, 3, B.P - 1, B.P - 4):
        r = G2W.f2_sqrt((a0, 0))
        assert r is not None and B.f2_sqr(r) == (a0, 0)
    assert G2W.f2_sqrt((B.P - 1, 0)) == (0, 1) and G2W.f2_sqrt((3, 0))[0] == 0   # -1 = u^2; 3 is not a square in Fq


def test_g2_codec_round_trips():
    rng = random.Random(4)
    pts = [B.G2, B.g2_neg(B.G2)] + [B.g2_mul(B.G2, s) for s in (2, 3, B.R - 1, rng.randrange(B.R), rng.randrange(B.R))]
    signs = set()
    for q in pts:
        b = G2W.compress(q)
        assert len(b) == 64 and b[63] & 0x40 == 0
        signs.add(b[63] >> 7)
        assert G2W.decompress(b) == (G2W.OK, q)
        assert G2W.check(q) == G2W.OK
    assert signs == {0, 1}                                  # both sign bits occur (Q and -Q differ in it)
    assert G2W.compress(None) == bytes(64) and G2W.decompress(bytes(64)) == (G2W.OK, None) and G2W.check(None) == G2W.OK
    # refusals: c0 >= p, c1 >= p (bit 6 of byte 63 is such a c1), an x with no root
    x0, x1 = B.G2[0]
    le = lambda v: v.to_bytes(32, "little")
    assert G2W.decompress(le(B.P) + le(x1))[0] == G2W.NOT_CANONICAL
    assert G2W.decompress(le(x0) + le(B.P))[0] == G2W.NOT_CANONICAL
    assert G2W.decompress(le(x0) + le(x1 | 1 << 254))[0] == G2W.NOT_CANONICAL
    x = G2W.x_without_root(rng)
    assert G2W.decompress(le(x[0]) + le(x[1])) == (G2W.OFF_TWIST, None)


def test_the_twist_has_points_outside_the_subgroup():
    """seed 1: a random twist point is not annihilated by r, and a point of order 10069 exists -- the cofactor 2p - r is not 1"""
    rng = random.Random(1)
    t = G2W.random_twist_point(rng)
    assert B.g2_on_curve(t) and B.g2_mul(t, B.R, reduce=False) is not None
    assert B.g2_mul(t, B.R * G2W.COFACTOR, reduce=False) is None          # the group order r (2p - r) does annihilate it
    assert G2W.check(t) == G2W.NOT_IN_SUBGROUP
    q = G2W.point_of_order_10069(random.Random(1))
    assert B.g2_on_curve(q) and q is not None and B.g2_mul(q, 10069, reduce=False) is None
    assert G2W.check(q) == G2W.NOT_IN_SUBGROUP
    assert G2W.decompress(G2W.compress(q)) == (G2W.OK, q)                 # the codec does not care about the subgroup


@pytest.fixture(scope="module")
def srs4():
    return PR.setup(4, 0x5EED5EED5EED)


def test_python_srs_is_one_srs(srs4):
    s, n, w = 0x5EED5EED5EED, 16, PR.omega(4)
    assert pow(w, 16, PR.R) == 1 and pow(w, 8, PR.R) != 1
    assert srs4.g[0] == (1, 2) and srs4.g[1] == W.mul(s) and srs4.g[15] == W.mul(pow(s, 15, PR.R))
    # sum_i L_i(X) = 1 and sum_i omega^i L_i(X) = X: the Lagrange points recombine to g[0] and g[1]
    acc0 = acc1 = None
    for i, p in enumerate(srs4.g_lagrange):
        acc0 = W.add(acc0, p)
        acc1 = W.add(acc1, W.mul(pow(w, i, PR.R), p))
    assert acc0 == srs4.g[0] and acc1 == srs4.g[1]
    assert srs4.g2 == B.G2 and srs4.s_g2 == B.g2_mul(B.G2, s)


def test_python_formats_round_trip(srs4):
    for fmt in (PR.PROCESSED, PR.RAW, PR.RAW_UNCHECKED):
        data = PR.encode(srs4, fmt)
        assert len(data) == PR.file_bytes(4, fmt)
        assert PR.decode(data, fmt) == srs4
    assert PR.encode(srs4, PR.RAW) == PR.encode(srs4, PR.RAW_UNCHECKED)
    assert PR.file_bytes(4, PR.RAW) == 4 + 2 * 64 * 16 + 256 and PR.file_bytes(4, PR.PROCESSED) == 4 + 2 * 32 * 16 + 128


def test_file_bytes_entry_point():
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import _lib, srs

    pz.build()
    L = pz.lib()
    n = C.c_size_t()
    for k in (4, 17, 26):
        for fmt in (_lib.PZ_SERDE_RAW, _lib.PZ_SERDE_RAW_UNCHECKED):
            assert L.pz_params_file_bytes(k, fmt, C.byref(n)) == 0 and n.value == srs.file_size(k)
        assert L.pz_params_file_bytes(k, _lib.PZ_SERDE_PROCESSED, C.byref(n)) == 0 and n.value == 4 + 2 * 32 * 2**k + 128
    assert PR.file_bytes(4, PR.RAW) == srs.file_size(4)
    for k, fmt in ((0, 1), (29, 1), (4, 3), (4, -1)):
        assert L.pz_params_file_bytes(k, fmt, C.byref(n)) == _lib.PZ_ERR_INVALID
    assert L.pz_params_file_bytes(4, 1, None) == _lib.PZ_ERR_INVALID
    assert (_lib.PZ_SERDE_PROCESSED, _lib.PZ_SERDE_RAW, _lib.PZ_SERDE_RAW_UNCHECKED) == (PR.PROCESSED, PR.RAW, PR.RAW_UNCHECKED) == (0, 1, 2)


def test_entry_points_are_exported_and_refuse_null():
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import _lib

    pz.build()
    L = pz.lib()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    h = C.c_void_p()
    inv = _lib.PZ_ERR_INVALID
    assert L.pz_g2_compress(None, p, 1, p) == inv and L.pz_g2_decompress(None, p, 1, p, p, None) == inv
    assert L.pz_g2_check_dev(None, p, 1, p) == inv and L.pz_g2_check(None, p, 1, p) == inv
    assert L.pz_params_decode(None, p, 512, 1, C.byref(h), None) == inv and not h.value
    assert L.pz_params_from_dev(None, 4, p, p, p, p, C.byref(h)) == inv
    assert L.pz_params_info(None, None, p, p, p) == inv and L.pz_params_points(None, None, None) == inv
    assert L.pz_params_bases(None, 0, C.byref(h)) == inv and L.pz_params_encode(None, 1, p, 512) == inv
    assert L.pz_params_downsize(None, 3, C.byref(h)) == inv and L.pz_params_check(None, None, None) == inv
    assert L.pz_params_free(None) == 0
    assert L.pz_abi_version() == 7


def build_params_tool(out_dir) -> str:
    csrc = os.path.join(ROOT, "paillier_halo2_amd", "csrc")
    exe = os.path.join(str(out_dir), "params_tool")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe,
                    os.path.join(ROOT, "paillier_halo2_amd", "host", "params_tool.cpp"), "-L" + csrc, "-lpz_hip", "-Wl,-rpath," + csrc,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_params_tool_builds_and_refuses_bad_input(tmp_path):
    import paillier_halo2_amd as pz

    pz.build()
    exe = build_params_tool(tmp_path)
    junk = tmp_path / "junk.srs"
    junk.write_bytes((7).to_bytes(4, "little") + b"\x01" * 64)            # a plausible k, the wrong size
    out = str(tmp_path / "out.srs")
    run = lambda *a: subprocess.run([exe, *a], capture_output=True, text=True)
    assert run().returncode == 2 and run("frobnicate", str(junk)).returncode == 2
    assert run("check").returncode == 2 and run("check", str(tmp_path / "absent.srs")).returncode == 2
    for args in (("check", str(junk)), ("convert", str(junk), "processed", out), ("downsize", str(junk), "5", out)):
        r = run(*args)
        assert r.returncode == 2 and "size" in r.stderr and not os.path.exists(out), (args, r.stderr)
    assert run("convert", str(junk), "cooked", out).returncode == 2      # an unknown format
    assert run("downsize", str(junk), "five", out).returncode == 2
