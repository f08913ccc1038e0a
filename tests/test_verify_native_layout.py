"""CPU: the device batch verifier's host-side pieces that need no GPU -- the ABI layout verifier.pack_proof writes (the stepper's outputs
in phase order, as pz_vk_info sizes them), and the compiled driver host/verify_connected.cpp builds against the C ABI alone and refuses
bad input before it touches a device."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_proof(A, Lk, S, rng):
    com = {f: rng.integers(0, 2 ** 63, size=(c, 8), dtype=np.uint64)
           for f, c in (("advice", A), ("lookup_advice", Lk), ("perm_inputs", Lk), ("perm_tables", Lk), ("perm_z", S), ("lookup_z", Lk),
                        ("random", 1), ("h", 3), ("w1", 1), ("w2", 1))}
    m = A + Lk + 1
    ev = {f: rng.integers(0, 2 ** 63, size=(c, p, 4), dtype=np.uint64)
          for f, c, p in (("advice", A, 4), ("lookup_advice", Lk, 1), ("constants", 1, 1), ("fixed", A + 2, 1), ("sigma", m, 1),
                          ("perm_z", S, 3), ("lookup_z", Lk, 2), ("perm_inputs", Lk, 2), ("perm_tables", Lk, 1), ("random", 1, 1),
                          ("h", 1, 1))}
    return com, ev


def test_pack_proof_is_the_stepper_layout():
    from paillier_halo2_amd import verifier as PV

    A, Lk = 5, 2
    m = A + Lk + 1
    S = -(-m // 2)
    vk = PV.VerifyingKey(14, 6, A, Lk, S, np.zeros((A + 2, 8), np.uint64), np.zeros((m, 8), np.uint64))
    com, ev = _fake_proof(A, Lk, S, np.random.default_rng(1))
    w = PV.pack_proof(vk, com, ev)
    cw = 8 * (A + 4 * Lk + S + 6)
    ew = 4 * (4 * A + (Lk + 1) + (A + 2) + m + 3 * S + 2 * Lk + 2 * Lk + Lk + 1 + 1)   # pz_pk_info's evals_words
    assert w.shape == (cw + ew,)
    off = 0
    for f in PV.PROOF_COMMITMENTS:
        n = com[f].size
        assert np.array_equal(w[off:off + n], com[f].reshape(-1)), f
        off += n
    assert off == cw
    for f in PV.PROOF_EVALS:
        n = ev[f].size
        assert np.array_equal(w[off:off + n], ev[f].reshape(-1)), f
        off += n
    assert off == cw + ew
    # the lookup-advice evaluations are followed by the constants row (pz_proof_evaluate's order), the h(x) element comes last
    assert np.array_equal(w[cw + 16 * A + 4 * Lk:cw + 16 * A + 4 * Lk + 4], ev["constants"].reshape(-1))
    assert np.array_equal(w[-4:], ev["h"].reshape(-1))
    bad = dict(com)
    bad["h"] = com["h"][:2]
    assert PV.pack_proof(vk, bad, ev) is None
    assert PV.pack_proof(vk, com, {k: v for k, v in ev.items() if k != "constants"}) is None


def test_compiled_driver_builds_and_refuses_bad_input(tmp_path):
    import paillier_halo2_amd as pz

    pz.build()
    csrc = os.path.join(ROOT, "paillier_halo2_amd", "csrc")
    exe = str(tmp_path / "verify_connected")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe,
                    os.path.join(ROOT, "paillier_halo2_amd", "host", "verify_connected.cpp"), "-L" + csrc, "-lpz_hip", "-Wl,-rpath," + csrc,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe], capture_output=True).returncode == 2
    junk = tmp_path / "junk.bin"
    junk.write_bytes(b"\x01" * 64)
    assert subprocess.run([exe, str(junk), str(junk), str(junk)], capture_output=True).returncode == 2
