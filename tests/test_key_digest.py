"""CPU: the verifying key's digest (include/pz.h pz_key_digest, host/key_digest.hpp; prover.key_digest) over synthetic
commitment words -- the library's BLAKE2b against hashlib's, what moves the digest, and the refusals.  No device is touched: pz_key_digest
takes no context."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import paillier_halo2_amd as pz
from paillier_halo2_amd import _lib, prover

SHAPE = dict(k=12, bf=6, n_adv=5, n_lk=2, n_instance=1, n_public=9)


def _words(n_points, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(n_points, 8), dtype=np.uint64)


def _key(**over):
    s = dict(SHAPE, **over)
    fixed = _words(s["n_adv"] + 2, 0x66697865)
    sigma = _words(s["n_adv"] + s["n_lk"] + 1 + s["n_instance"], 0x7369676d)
    return s, fixed, sigma


def lib_digest(s, fixed, sigma):
    out = (C.c_uint8 * 64)()
    f, g = np.ascontiguousarray(fixed, dtype=np.uint64), np.ascontiguousarray(sigma, dtype=np.uint64)
    rc = pz.lib().pz_key_digest(s["k"], s["bf"], s["n_adv"], s["n_lk"], s["n_instance"], s["n_public"], f.ctypes.data, g.ctypes.data, out)
    assert rc == _lib.PZ_OK
    return bytes(out)


def ref_digest(s, fixed, sigma):
    """the definition, written out: BLAKE2b-512 personalised PZ-Key-Digest-v1 over six little-endian u64, then the words of fixed and sigma"""
    h = hashlib.blake2b(digest_size=64, person=b"PZ-Key-Digest-v1")
    h.update(struct.pack("<6Q", s["k"], s["bf"], s["n_adv"], s["n_lk"], s["n_instance"], s["n_public"]))
    for arr in (fixed, sigma):
        for w in np.asarray(arr, dtype=np.uint64).reshape(-1):
            h.update(struct.pack("<Q", int(w)))
    return h.digest()


def py_digest(s, fixed, sigma):
    return prover.key_digest(s["k"], s["bf"], s["n_adv"], s["n_lk"], fixed, sigma, s["n_instance"], s["n_public"])


@pytest.mark.parametrize("over", [dict(), dict(n_instance=0, n_public=0), dict(n_adv=1, n_lk=1, n_instance=0, n_public=0),
                                  dict(k=17, n_adv=37, n_lk=5, n_instance=0, n_public=0)])
def test_library_hashlib_and_python_agree(over):
    s, fixed, sigma = _key(**over)
    want = ref_digest(s, fixed, sigma)
    assert len(want) == 64
    assert lib_digest(s, fixed, sigma) == want
    assert py_digest(s, fixed, sigma) == want
    # the input is (2 n_adv + n_lk + 3 + n_instance) points of 64 bytes behind the 48-byte shape
    assert 48 + fixed.nbytes + sigma.nbytes == 48 + 64 * (2 * s["n_adv"] + s["n_lk"] + 3 + s["n_instance"])


def test_every_shape_integer_moves_the_digest():
    s, fixed, sigma = _key()
    base = lib_digest(s, fixed, sigma)
    seen = {base}
    # one integer at a time, the buffers the same (oversized, so that a larger count still reads inside them)
    big_f, big_s = _words(16, 0x66697865), _words(16, 0x7369676d)
    assert np.array_equal(big_f[:7], fixed) and np.array_equal(big_s[:9], sigma) and lib_digest(s, big_f, big_s) == base
    for name in ("k", "bf", "n_adv", "n_lk", "n_instance", "n_public"):
        for step in (1, -1):
            t = dict(s, **{name: s[name] + step})
            if not t["n_instance"]:
                continue                            # (n_public without the column is refused: below)
            d = lib_digest(t, big_f, big_s)
            assert d not in seen and d == ref_digest(t, big_f[:t["n_adv"] + 2], big_s[:t["n_adv"] + t["n_lk"] + 1 + t["n_instance"]]), (name, step)
            seen.add(d)
    assert lib_digest(dict(s, n_instance=0, n_public=0), fixed, sigma) not in seen
    # n_adv and n_lk are told apart although both only shift the boundary between the arrays: same bytes hashed, another shape in front
    a = dict(s, n_adv=4, n_lk=4)                    # fixed 6 points, sigma 10: the arrays of s (7 and 9) hold enough
    whole = np.concatenate([fixed, sigma])
    assert lib_digest(a, whole[:6], whole[6:]) != base
    assert py_digest(dict(s, n_instance=0, n_public=0), fixed, sigma[:-1]) == lib_digest(dict(s, n_instance=0, n_public=0), fixed, sigma[:-1])


def test_every_commitment_word_and_their_order_move_the_digest():
    s, fixed, sigma = _key()
    base = lib_digest(s, fixed, sigma)
    for which, arr in (("fixed", fixed), ("sigma", sigma)):
        for point, word in ((0, 0), (arr.shape[0] - 1, 7), (2, 3)):
            t = arr.copy()
            t[point, word] ^= np.uint64(1)
            args = (t, sigma) if which == "fixed" else (fixed, t)
            d = lib_digest(s, *args)
            assert d != base and d == ref_digest(s, *args), (which, point, word)
    for which, arr in (("fixed", fixed), ("sigma", sigma)):
        t = arr.copy()
        t[[0, 1]] = t[[1, 0]]
        args = (t, sigma) if which == "fixed" else (fixed, t)
        assert lib_digest(s, *args) != base, which
    # the last fixed commitment against the first sigma commitment: the boundary between the arrays
    f2, s2 = fixed.copy(), sigma.copy()
    f2[-1], s2[0] = sigma[0], fixed[-1]
    assert lib_digest(s, f2, s2) != base


def test_bad_arguments_are_refused():
    L = pz.lib()
    s, fixed, sigma = _key()
    out = (C.c_uint8 * 64)()
    f, g = fixed.ctypes.data, sigma.ctypes.data
    args = (s["k"], s["bf"], s["n_adv"], s["n_lk"], s["n_instance"], s["n_public"])
    assert L.pz_key_digest(*args, f, g, out) == _lib.PZ_OK
    assert L.pz_key_digest(*args, None, g, out) == _lib.PZ_ERR_INVALID
    assert L.pz_key_digest(*args, f, None, out) == _lib.PZ_ERR_INVALID
    assert L.pz_key_digest(*args, f, g, None) == _lib.PZ_ERR_INVALID
    assert L.pz_key_digest(s["k"], s["bf"], s["n_adv"], s["n_lk"], 0, 3, f, g, out) == _lib.PZ_ERR_INVALID      # public values without the column
    assert L.pz_key_digest(s["k"], s["bf"], s["n_adv"], s["n_lk"], 0, 0, f, g, out) == _lib.PZ_OK
    # the object forms refuse a null key (no device needed to say so)
    on = C.c_int(7)
    assert L.pz_pk_digest(None, out) == _lib.PZ_ERR_INVALID and L.pz_vk_digest(None, out) == _lib.PZ_ERR_INVALID
    assert L.pz_vk_bind(None, 1) == _lib.PZ_ERR_INVALID and L.pz_vk_is_bound(None, C.byref(on)) == _lib.PZ_ERR_INVALID and on.value == 7
    with pytest.raises(ValueError):
        prover.key_digest(12, 6, 5, 2, fixed, sigma[:-2], 1, 9)
    with pytest.raises(ValueError):
        prover.key_digest(12, 6, 5, 2, fixed, sigma[:-1], 0, 3)


def test_a_bound_transcript_is_the_unbound_one_over_digest_then_seed():
    s, fixed, sigma = _key()
    D = py_digest(s, fixed, sigma)
    pts = _words(3, 1)
    bound, plain, glued = prover.HashTranscript(b"seed", key_digest=D), prover.HashTranscript(b"seed"), prover.HashTranscript(D + b"seed")
    for t in (bound, plain, glued):
        t.absorb_affine(pts)
        t.squeeze("theta")
    assert bound.drawn == glued.drawn != plain.drawn
    assert bound.seed == plain.seed == b"seed" and bound.key_digest == D and plain.key_digest is None
    with pytest.raises(ValueError):
        prover.HashTranscript(b"seed", key_digest=D[:32])


def test_the_drivers_headers_give_the_same_digest_and_bound_transcript(tmp_path):
    """host/key_digest.hpp and host/transcript.hpp as a compiled driver includes them (no library), against hashlib and prover.py"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "key_digest_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(here, "cpp", "key_digest_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {ln.split()[0]: ln.split()[1] for ln in out.splitlines()}
    M64 = (1 << 64) - 1
    s = dict(SHAPE)
    fixed = np.array([(0x9E3779B97F4A7C15 * (i + 1)) & M64 for i in range(8 * 7)], dtype=np.uint64).reshape(7, 8)
    sigma = np.array([(0xBF58476D1CE4E5B9 * (i + 3)) & M64 for i in range(8 * 9)], dtype=np.uint64).reshape(9, 8)
    D = ref_digest(s, fixed, sigma)
    assert got["digest"] == D.hex() == py_digest(s, fixed, sigma).hex() == lib_digest(s, fixed, sigma).hex()
    seed = (5).to_bytes(8, "little")
    for name, tr in (("bound", prover.HashTranscript(seed, key_digest=D)), ("plain", prover.HashTranscript(seed))):
        tr.absorb_affine(fixed[:3])
        a = tr.squeeze("a")
        tr.absorb_scalars(sigma.reshape(-1, 4)[:2])
        b = tr.squeeze("b")
        assert int.from_bytes(bytes.fromhex(got[name + "_a"]), "little") == a, name
        assert int.from_bytes(bytes.fromhex(got[name + "_b"]), "little") == b, name
    assert got["bound_a"] != got["plain_a"]
