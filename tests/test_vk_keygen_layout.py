"""CPU: keygen_vk's surface that needs no GPU -- the four entry points (pz_g1_commit_mask_dev, pz_permutation_sigma_part_dev,
pz_vk_keygen_dev, pz_vk_keygen) are declared, exported and bound; each refuses a NULL context; and the compiled driver host/keygen_vk.cpp
builds against the C ABI alone and refuses bad input before it touches a device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pz_g1_commit_mask_dev", "pz_permutation_sigma_part_dev", "pz_vk_keygen_dev", "pz_vk_keygen")


def test_entry_points_are_declared_exported_and_bound():
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import _lib

    pz.build()
    L = pz.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pz.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    crate = open(os.path.join(ROOT, "rust", "pz-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name + " is not declared in include/pz.h"
        assert hasattr(L, name) and name in _lib.SIGNATURES, name + " is not exported / has no ctypes signature"
        assert ("pub fn %s(" % name) in doc, name + " has no binding in INTEGRATION.md"
        assert ("pub fn %s(" % name) in crate, name + " has no binding in rust/pz-sys"
    assert L.pz_abi_version() == 7


def test_null_context_is_invalid():
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import _lib

    pz.build()
    L = pz.lib()
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.pz_g1_commit_mask_dev(None, p, p, 1, 16, 16, p) == _lib.PZ_ERR_INVALID
    assert L.pz_permutation_sigma_part_dev(None, p, p, 3, 0, 1, 4, p, p, p, 64) == _lib.PZ_ERR_INVALID
    for fn in (L.pz_vk_keygen_dev, L.pz_vk_keygen):
        assert fn(None, p, 4, 2, 1, 1, p, p, 1, p, p, 0, p, p) == _lib.PZ_ERR_INVALID


def test_compiled_driver_builds_and_refuses_bad_input(tmp_path):
    import paillier_halo2_amd as pz

    pz.build()
    csrc = os.path.join(ROOT, "paillier_halo2_amd", "csrc")
    exe = str(tmp_path / "keygen_vk")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-o", exe,
                    os.path.join(ROOT, "paillier_halo2_amd", "host", "keygen_vk.cpp"), "-L" + csrc, "-lpz_hip", "-Wl,-rpath," + csrc,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = str(tmp_path / "out.vk")
    assert subprocess.run([exe], capture_output=True).returncode == 2
    assert subprocess.run([exe, "a", "b", "c"], capture_output=True).returncode == 2
    junk = tmp_path / "junk.srs"
    junk.write_bytes((14).to_bytes(4, "little") + b"\x01" * 64)         # the right k, the wrong size
    shape = ["128", "64", "13", "14", "20", "6"]
    r = subprocess.run([exe, str(junk), "encrypt", *shape, "1f", "2b", out], capture_output=True)
    assert r.returncode == 2 and not os.path.exists(out)
    r = subprocess.run([exe, str(junk), "add", *shape, out], capture_output=True)
    assert r.returncode == 2 and not os.path.exists(out)
    # malformed shapes are refused before any file is read
    assert subprocess.run([exe, str(junk), "multiply", *shape, out], capture_output=True).returncode == 2
    assert subprocess.run([exe, str(junk), "encrypt", *shape, "xyz", "2b", out], capture_output=True).returncode == 2
    assert subprocess.run([exe, str(junk), "encrypt", *shape, out], capture_output=True).returncode == 2     # encrypt without its exponents
