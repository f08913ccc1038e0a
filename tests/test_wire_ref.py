"""CPU: the halo2 wire format as tests/wire_ref.py states it -- known answers derivable by hand, round trips,
refusals, the proof size, the wire order against verifier.PROOF_COMMITMENTS / PROOF_EVALS -- and the compiled driver host/verify_wire.cpp
builds against the C ABI alone and refuses bad input before it touches a device.  The device codec is checked against this reference by
tests/test_gpu_wire.py."""
import os
import random
import subprocess

import numpy as np

from tests import wire_ref as WR
from tests.util import H, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _expected(x, y):
    """what the format says, spelled without wire_ref: x little-endian, the top bit of byte 31 = the parity of y"""
    b = bytearray(x.to_bytes(32, "little"))
    b[31] |= (y & 1) << 7
    return bytes(b)


def test_known_answers():
    assert WR.compress((1, 2)) == bytes([1]) + bytes(31)
    assert WR.compress((1, WR.P - 2)) == bytes([1]) + bytes(30) + bytes([0x80])       # p - 2 is odd
    assert WR.compress(None) == bytes(32)
    assert WR.decompress(bytes([1]) + bytes(31)) == (WR.OK, (1, 2))
    assert WR.decompress(bytes([1]) + bytes(30) + bytes([0x80])) == (WR.OK, (1, WR.P - 2))
    assert WR.decompress(bytes(32)) == (WR.OK, None)
    k = load_golden("external_kats.json")
    pts = []
    for v in k["ecadd"]:
        pts += [(H(v["x1"]), H(v["y1"])), (H(v["x2"]), H(v["y2"])), (H(v["x3"]), H(v["y3"]))]
    for v in k["ecmul"]:
        pts += [(H(v["x"]), H(v["y"])), (H(v["x3"]), H(v["y3"]))]
    assert WR.mul(2) in pts and WR.mul(9) in pts                                           # 2G and 9G are among the published points
    seen = 0
    for x, y in pts:
        if (x, y) == (0, 0):
            continue
        seen += 1
        b = WR.compress((x, y))
        assert b == _expected(x, y) and b[31] & 0x40 == 0
        assert WR.decompress(b) == (WR.OK, (x, y))
    assert seen >= 10


def test_round_trip_of_random_multiples():
    rng = random.Random(0x77697265)
    parities = set()
    for _ in range(256):
        pt = WR.mul(rng.randrange(1, WR.R))
        b = WR.compress(pt)
        parities.add(b[31] >> 7)
        assert WR.decompress(b) == (WR.OK, pt)
        assert WR.points_from_words(WR.point_words(pt)) == [pt]
    assert parities == {0, 1}


def test_refusals():
    assert WR.decompress(WR.P.to_bytes(32, "little")) == (WR.NOT_CANONICAL, None)                  # x = p
    assert WR.decompress((1 | 1 << 254).to_bytes(32, "little")) == (WR.NOT_CANONICAL, None)        # bit 6 of byte 31
    assert WR.decompress((1 << 255).to_bytes(32, "little")) == (WR.OFF_CURVE, None)                # x = 0 with sign 1
    rng = random.Random(0x6f6666)
    off = [x for x in (rng.randrange(WR.P) for _ in range(64)) if pow((x ** 3 + 3) % WR.P, (WR.P - 1) // 2, WR.P) != 1]
    assert 16 < len(off) < 48                                                                      # about half of all x
    for x in off:
        assert WR.decompress(x.to_bytes(32, "little")) == (WR.OFF_CURVE, None)
        assert WR.decompress((x | 1 << 255).to_bytes(32, "little")) == (WR.OFF_CURVE, None)
    assert WR.scalar_from_bytes(WR.R.to_bytes(32, "little")) == (WR.NOT_CANONICAL, None)
    assert WR.scalar_from_bytes((WR.R - 1).to_bytes(32, "little")) == (WR.OK, WR.R - 1)


def test_random_strings_fall_in_three_classes():
    """the shares tests/test_gpu_wire.py relies on: ~62 % not canonical, ~19 % off the curve, ~19 % accepted"""
    rng = random.Random(0x72656675)
    cls = [WR.decompress(rng.randbytes(32))[0] for _ in range(512)]
    n = [cls.count(c) for c in (WR.OK, WR.NOT_CANONICAL, WR.OFF_CURVE)]
    assert 60 < n[0] < 140 and 270 < n[1] < 370 and 60 < n[2] < 140, n


def test_proof_size_formula():
    from paillier_halo2_amd import verifier as PV

    assert WR.proof_counts(3034, 84) == (4936, 23478)                  # config c2
    assert WR.proof_size(3034, 84) == 32 * (4936 + 23477) == 909216
    assert 8 * (8 * 4936 + 4 * 23478) == 1067200                        # the word layout of the same proof
    for A, Lk in ((3034, 84), (5, 2), (6, 1), (1, 1)):
        m = A + Lk + 1
        vk = PV.VerifyingKey(14, 6, A, Lk, -(-m // 2), np.zeros((A + 2, 8), np.uint64), np.zeros((m, 8), np.uint64))
        assert PV.proof_size_bytes(vk) == WR.proof_size(A, Lk)


def _fake_proof(A, Lk, S, rng):
    """prover.Proof-shaped arrays with real curve points and canonical scalars"""
    mont = lambda v: [(v * WR.MONT % WR.R >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]
    pts = lambda c: np.array([WR.point_words(WR.mul(rng.randrange(1, 1 << 16))) for _ in range(c)], dtype=np.uint64).reshape(c, 8)
    com = {f: pts(c) for f, c in (("advice", A), ("lookup_advice", Lk), ("perm_inputs", Lk), ("perm_tables", Lk), ("perm_z", S),
                                  ("lookup_z", Lk), ("random", 1), ("h", 3), ("w1", 1), ("w2", 1))}
    m = A + Lk + 1
    ev = {f: np.array([mont(rng.randrange(WR.R)) for _ in range(c * p)], dtype=np.uint64).reshape(c, p, 4)
          for f, c, p in (("advice", A, 4), ("lookup_advice", Lk, 1), ("constants", 1, 1), ("fixed", A + 2, 1), ("sigma", m, 1),
                          ("perm_z", S, 3), ("lookup_z", Lk, 2), ("perm_inputs", Lk, 2), ("perm_tables", Lk, 1), ("random", 1, 1),
                          ("h", 1, 1))}
    return com, ev


def test_wire_order_is_the_absorption_order():
    """the reference's packing against verifier.PROOF_COMMITMENTS / PROOF_EVALS: the word layout's families in order, W1 and W2 moved behind
    the evaluations, h(x) dropped"""
    from paillier_halo2_amd import verifier as PV

    A, Lk = 5, 2
    m = A + Lk + 1
    S = -(-m // 2)
    com, ev = _fake_proof(A, Lk, S, random.Random(2))
    data = WR.proof_bytes(com, ev)
    assert len(data) == WR.proof_size(A, Lk)
    assert PV.PROOF_COMMITMENTS[-2:] == ("w1", "w2") and PV.PROOF_EVALS[-1] == "h"
    want = []
    for f in PV.PROOF_COMMITMENTS[:-2]:
        want += [WR.compress(p) for p in WR.points_from_words(com[f])]
    for f in PV.PROOF_EVALS[:-1]:
        want += [v.to_bytes(32, "little") for v in WR.scalars_from_words(ev[f])]
    for f in ("w1", "w2"):
        want += [WR.compress(p) for p in WR.points_from_words(com[f])]
    assert [data[i:i + 32] for i in range(0, len(data), 32)] == want
    # the same count as the word layout minus the h(x) element
    vk = PV.VerifyingKey(14, 6, A, Lk, S, np.zeros((A + 2, 8), np.uint64), np.zeros((m, 8), np.uint64))
    words = PV.pack_proof(vk, com, ev)
    n_own, n_ev = WR.proof_counts(A, Lk)
    assert words.shape == (8 * n_own + 4 * n_ev,) and len(want) == n_own + n_ev - 1


def test_vk_file_layout():
    A, Lk = 3, 1
    rng = random.Random(3)
    pts = lambda c: np.array([WR.point_words(WR.mul(rng.randrange(1, 1 << 16))) for _ in range(c)], dtype=np.uint64)
    fixed, sigma = pts(A + 2), pts(A + Lk + 1)
    b = WR.vk_bytes(14, 6, A, Lk, fixed, sigma)
    assert b[:4] == b"PZVK" and len(b) == 24 + 32 * (2 * A + Lk + 3)
    assert np.frombuffer(b[4:24], dtype="<u4").tolist() == [1, 14, 6, A, Lk]
    assert WR.decompress(b[24:56])[1] == WR.points_from_words(fixed[0])[0]


def test_compiled_wire_driver_builds_and_refuses_bad_input(tmp_path):
    import paillier_halo2_amd as pz

    pz.build()
    csrc = os.path.join(ROOT, "paillier_halo2_amd", "csrc")
    exe = str(tmp_path / "verify_wire")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe,
                    os.path.join(ROOT, "paillier_halo2_amd", "host", "verify_wire.cpp"), "-L" + csrc, "-lpz_hip", "-Wl,-rpath," + csrc,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe], capture_output=True).returncode == 2
    junk = tmp_path / "junk.bin"
    junk.write_bytes(b"\x01" * 64)
    assert subprocess.run([exe, str(junk), str(junk), str(junk)], capture_output=True).returncode == 2
