"""GPU: ParamsKZG files through the C ABI (include/pz.h: pz_g2_compress / pz_g2_decompress / pz_g2_check[_dev], pz_params_*; srs.load_params /
srs.Params; host/params_tool.cpp) against the Python-integer references tests/g2_wire_ref.py and tests/params_ref.py: the 64-byte G2 codec
byte for byte and word for word, the subgroup check on twist points outside the order-r subgroup, the three file formats at k = 4 against
an SRS built in Python, round trips and refusals at k = 7 across ragged chunk boundaries (PZ_PARAMS_CHUNK = 48), every verdict bit of
pz_params_check on a tampered SRS, downsize, the object's base tables, and the compiled driver."""
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests import bn254_pairing_ref as B
from tests import g2_wire_ref as G2W
from tests import params_ref as PR
from tests import wire_ref as W
from tests.test_params_ref import build_params_tool

pytestmark = pytest.mark.gpu

S = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA987654321          # the toxic scalar of the tests' SRS
S_OTHER = 0x0BADC0DE0BADC0DE0BADC0DE
G1B, G2B, G0B, POWERS, LAGRANGE = 1, 2, 4, 8, 16
PROCESSED, RAW, RAW_UNCHECKED = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def small_chunks():
    """48 points per chunk: the 128 points of a k = 7 section are decoded and encoded as 48 + 48 + 32"""
    old = os.environ.get("PZ_PARAMS_CHUNK")
    os.environ["PZ_PARAMS_CHUNK"] = "48"
    yield
    if old is None:
        del os.environ["PZ_PARAMS_CHUNK"]
    else:
        os.environ["PZ_PARAMS_CHUNK"] = old


@pytest.fixture(scope="module")
def eng(small_chunks):
    import paillier_halo2_amd as pz

    e = pz.Engine(0)
    yield e
    e.close()


def fr(v):
    return np.array(B.fr_words(v), dtype=np.uint64)


def g2w(q):
    return np.array(B.g2_words(q), dtype=np.uint64)


def device_setup(eng, k, s, s_g2_scalar=None):
    """(g, g_lagrange) as host arrays (2^k, 8) and (g2, s_g2) as 128 bytes each: pz_srs_setup_g1_dev and srs.setup_g2"""
    from paillier_halo2_amd import srs

    n = 1 << k
    d = eng.dev_alloc(2 * n * 64)
    try:
        eng.srs_setup_g1_dev(k, fr(s), fr(PR.omega(k)), d, d + n * 64)
        g, gl = eng.download(d, (n, 8)), eng.download(d + n * 64, (n, 8))
    finally:
        eng.dev_free(d)
    g2, s_g2 = srs.setup_g2(eng, fr(s if s_g2_scalar is None else s_g2_scalar))
    return g, gl, g2, s_g2


def make_params(eng, k, g, gl, g2, s_g2):
    """a params object from host arrays (gl = None: derived on the device)"""
    from paillier_halo2_amd import srs

    n = 1 << k
    d = eng.dev_alloc(2 * n * 64)
    try:
        eng.upload(d, np.ascontiguousarray(g, dtype=np.uint64))
        if gl is not None:
            eng.upload(d + n * 64, np.ascontiguousarray(gl, dtype=np.uint64))
        return srs.Params.from_dev(eng, k, d, 0 if gl is None else d + n * 64, g2, s_g2)
    finally:
        eng.dev_free(d)


@pytest.fixture(scope="module")
def world7(eng):
    g, gl, g2, s_g2 = device_setup(eng, 7, S)
    p = make_params(eng, 7, g, gl, g2, s_g2)
    raw = p.handle.encode(RAW).tobytes()
    yield {"g": g, "gl": gl, "g2": g2, "s_g2": s_g2, "params": p, "raw": raw}
    p.free()


def names(bits):
    return {n for b, n in ((G1B, "BAD_G1"), (G2B, "BAD_G2"), (G0B, "BAD_G0"), (POWERS, "BAD_POWERS"), (LAGRANGE, "BAD_LAGRANGE")) if bits & b}


# ---------------------------------------------------------------------------------------------------------------- the G2 kernels
def test_g2_codec_matches_reference(eng):
    rng = random.Random(21)
    pts = [B.G2, B.g2_neg(B.G2), None] + [B.g2_mul(B.G2, s) for s in (2, B.R - 1, S, rng.randrange(B.R), rng.randrange(B.R), rng.randrange(B.R))]
    pts.append(G2W.point_of_order_10069(random.Random(1)))       # the codec does not ask for the subgroup
    words = np.array([B.g2_words(q) for q in pts], dtype=np.uint64)
    want = b"".join(G2W.compress(q) for q in pts)
    got = eng.g2_compress(words)
    assert got.shape == (len(pts), 64) and got.tobytes() == want
    assert {b[63] >> 7 for b in got} == {0, 1}
    back, st = eng.g2_decompress(want)
    assert st.tolist() == [0] * len(pts) and np.array_equal(back, words)
    for i, q in enumerate(pts):
        assert B.g2_from_words(back[i]) == q == G2W.decompress(want[64 * i: 64 * i + 64])[1]
    # refusals, each beside a good point: an x with no root (2), c0 >= p and c1 >= p (1; bit 6 of byte 63 is such a c1)
    le = lambda v: v.to_bytes(32, "little")
    x0, x1 = B.G2[0]
    nx = G2W.x_without_root(rng)
    bad = [le(nx[0]) + le(nx[1]), le(nx[0]) + le(nx[1] | 1 << 255), le(B.P) + le(x1), le(x0) + le(B.P), le(x0) + le(x1 | 1 << 254),
           le((1 << 256) - 1) + le(x1)]
    data = b"".join(b + G2W.compress(B.G2) for b in bad)
    back, st = eng.g2_decompress(data)
    assert st.tolist() == [v for b in bad for v in (G2W.decompress(b)[0], 0)] == [2, 0, 2, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    for i in range(len(bad)):
        assert not back[2 * i].any() and np.array_equal(back[2 * i + 1], words[0])      # a refused point is the identity


def test_g2_check_tells_the_subgroup_from_the_twist(eng):
    rng = random.Random(1)
    t = G2W.random_twist_point(rng)
    q = G2W.point_of_order_10069(random.Random(1))
    off = (B.G2[0], (B.G2[1][0] + 1, B.G2[1][1]))
    good = [B.G2, B.g2_mul(B.G2, S), B.g2_mul(B.G2, B.R - 1), B.g2_neg(B.G2), None]
    words = np.array([B.g2_words(p) for p in good + [t, q, off]] + [B.g2_words(B.G2)] * 2, dtype=np.uint64)
    words[-2, 0:4] = [0xFFFFFFFFFFFFFFFF] * 3 + [0x3FFFFFFFFFFFFFFF]            # x.c0 above p
    words[-1, 12:16] = [int(v) for v in struct.unpack("<4Q", B.P.to_bytes(32, "little"))]   # y.c1 = p exactly
    want = [0] * 5 + [3, 3, 2, 1, 1]
    assert [G2W.check(p) for p in good + [t, q, off]] == want[:8]
    assert eng.g2_check(words).tolist() == want
    # the device-pointer form
    n = words.shape[0]
    d = eng.dev_alloc(n * 128 + n * 4)
    try:
        eng.upload(d, words)
        eng.g2_check_dev(d, n, d + n * 128)
        assert eng.download(d + n * 128, n, np.int32).tolist() == want
    finally:
        eng.dev_free(d)


# ---------------------------------------------------------------------------------------------------------------- formats
def test_setup_at_k4_equals_the_python_srs_in_all_encodings(eng):
    ref = PR.setup(4, S)
    g, gl, g2, s_g2 = device_setup(eng, 4, S)
    p = make_params(eng, 4, g, gl, g2, s_g2)
    derived = make_params(eng, 4, g, None, g2, s_g2)            # g_lagrange from g alone
    try:
        for fmt in (PROCESSED, RAW, RAW_UNCHECKED):
            want = PR.encode(ref, fmt)
            assert p.handle.encode(fmt).tobytes() == want, fmt
            assert derived.handle.encode(fmt).tobytes() == want, fmt
            # and the reference's bytes decode to the same object
            q = eng.params_decode(want, fmt)
            try:
                assert q.k == 4 and q.encode(RAW).tobytes() == PR.encode(ref, RAW)
                assert q.check() == (0, 0)
            finally:
                q.free()
        assert p.check() == (set(), set())
    finally:
        p.free()
        derived.free()


def test_round_trips_at_k7_and_sizes(eng, world7, tmp_path):
    from paillier_halo2_amd import _lib, srs

    p, raw = world7["params"], world7["raw"]
    # RAW is srs.write_params_kzg's file
    path = str(tmp_path / "kzg_bn254_7.srs")
    srs.write_params_kzg(path, 7, world7["g"], world7["gl"], world7["g2"], world7["s_g2"])
    assert open(path, "rb").read() == raw and len(raw) == srs.file_size(7)
    enc = {fmt: p.handle.encode(fmt).tobytes() for fmt in (PROCESSED, RAW, RAW_UNCHECKED)}
    assert enc[RAW] == enc[RAW_UNCHECKED] == raw and len(enc[PROCESSED]) == 4 + 2 * 32 * 128 + 128
    for a in (PROCESSED, RAW, RAW_UNCHECKED):
        q = eng.params_decode(enc[a], a)
        try:
            for b in (PROCESSED, RAW, RAW_UNCHECKED):
                assert q.encode(b).tobytes() == enc[b], (a, b)
        finally:
            q.free()
    # srs.load_params takes the format from the size; Params.write writes either
    ppath = str(tmp_path / "processed.srs")
    p.write(ppath, "processed")
    assert open(ppath, "rb").read() == enc[PROCESSED]
    for f in (path, ppath):
        q = srs.load_params(eng, f)
        try:
            assert q.k == 7 and q.handle.encode(RAW).tobytes() == raw and q.check() == (set(), set())
        finally:
            q.free()
    # a wrong length, a k outside 1..28 and an unknown format are refused, with no point counted
    for data, fmt in ((raw[:-1], RAW), (raw + b"\0", RAW), (raw, PROCESSED), (enc[PROCESSED], RAW), (raw[:3], RAW),
                      (struct.pack("<I", 29) + raw[4:], RAW), (struct.pack("<I", 0) + raw[4:], RAW_UNCHECKED), (raw, 3)):
        with pytest.raises(_lib.PzError) as e:
            eng.params_decode(data, fmt)
        assert e.value.status == _lib.PZ_ERR_INVALID and e.value.n_bad == 0
    # too small an output
    out = np.zeros(len(raw) - 1, dtype=np.uint8)
    assert eng.L.pz_params_encode(p.handle.handle, RAW, out.ctypes.data, out.size) == _lib.PZ_ERR_CAPACITY


def test_a_point_off_the_curve_is_refused_or_reported(eng, world7):
    from paillier_halo2_amd import _lib

    p, raw = world7["params"], world7["raw"]
    proc = bytearray(p.handle.encode(PROCESSED).tobytes())
    rng = random.Random(22)
    while True:                                                  # an x with no y
        x = rng.randrange(W.P)
        if W.decompress(x.to_bytes(32, "little"))[0] == W.OFF_CURVE:
            break
    for idx in (3, 100, 128 + 47, 128 + 48):                     # g and g_lagrange, first / last chunk, both sides of a chunk boundary
        bad = bytearray(proc)
        bad[4 + 32 * idx: 4 + 32 * idx + 32] = x.to_bytes(32, "little")
        with pytest.raises(_lib.PzError) as e:
            eng.params_decode(bytes(bad), PROCESSED)
        assert e.value.status == _lib.PZ_ERR_INVALID and e.value.n_bad == 1, idx
    # a G2 point off the twist
    bad = bytearray(proc)
    nx = G2W.x_without_root(rng)
    bad[-64:] = nx[0].to_bytes(32, "little") + nx[1].to_bytes(32, "little")
    with pytest.raises(_lib.PzError) as e:
        eng.params_decode(bytes(bad), PROCESSED)
    assert e.value.n_bad == 1
    # the same in raw bytes: (x, y + 1) in place of g[100]
    (pt,) = W.points_from_words(world7["g"][100])
    bad = bytearray(raw)
    bad[4 + 64 * 100: 4 + 64 * 101] = b"".join(struct.pack("<Q", w) for w in W.point_words((pt[0], (pt[1] + 1) % W.P)))
    with pytest.raises(_lib.PzError) as e:
        eng.params_decode(bytes(bad), RAW)
    assert e.value.status == _lib.PZ_ERR_INVALID and e.value.n_bad == 1
    q = eng.params_decode(bytes(bad), RAW_UNCHECKED)            # sizes only
    try:
        assert q.encode(RAW).tobytes() == bytes(bad)
        failed, skipped = q.check()
        assert failed == G1B and skipped == POWERS | LAGRANGE    # nothing unchecked reaches an MSM or the pairing
    finally:
        q.free()


# ---------------------------------------------------------------------------------------------------------------- check
def test_check_names_each_tamper(eng, world7):
    from paillier_halo2_amd import srs

    g, gl, g2, s_g2, n = world7["g"], world7["gl"], world7["g2"], world7["s_g2"], 128
    assert world7["params"].handle.check() == (0, 0)
    assert world7["params"].check() == (set(), set())

    def verdict(g_, gl_, g2_, s_g2_):
        p = make_params(eng, 7, g_, gl_, g2_, s_g2_)
        try:
            return p.handle.check()
        finally:
            p.free()

    def with_g(i, j):
        t = g.copy()
        t[i] = g[j]
        return t

    # a break inside the sequence, and at its last index: POWERS (g_lagrange is then not g's Lagrange form either)
    for t in (with_g(5, 6), with_g(n - 1, 0)):
        failed, skipped = verdict(t, gl, g2, s_g2)
        assert failed & POWERS and not failed & ~(POWERS | LAGRANGE) and skipped == 0, names(failed)
    # two Lagrange points swapped: LAGRANGE only
    t = gl.copy()
    t[[9, 77]] = gl[[77, 9]]
    assert verdict(g, t, g2, s_g2) == (LAGRANGE, 0)
    # s_g2 = [s + 1] g2, and a G2 side from another setup altogether: POWERS only
    _, other = srs.setup_g2(eng, fr(S + 1))
    assert verdict(g, gl, g2, other) == (POWERS, 0)
    _, other = srs.setup_g2(eng, fr(S_OTHER))
    assert verdict(g, gl, g2, other) == (POWERS, 0)
    # g2 outside the order-r subgroup: BAD_G2, and the pairing never sees it
    twist = g2w(G2W.random_twist_point(random.Random(1))).astype("<u8").tobytes()
    assert verdict(g, gl, twist, s_g2) == (G2B, POWERS | LAGRANGE)
    small = g2w(G2W.point_of_order_10069(random.Random(1))).astype("<u8").tobytes()
    assert verdict(g, gl, g2, small) == (G2B, POWERS | LAGRANGE)
    assert verdict(g, gl, bytes(128), s_g2) == (G2B, POWERS | LAGRANGE)          # the identity is no g2
    # a geometric sequence from the identity: g[i] = [s^i] O
    zero = np.zeros_like(g)
    assert verdict(zero, zero, g2, s_g2) == (G0B, POWERS | LAGRANGE)


# ---------------------------------------------------------------------------------------------------------------- downsize, bases, info
def test_downsize_equals_the_smaller_setup(eng, world7):
    from paillier_halo2_amd import _lib

    g5, gl5, g2, s_g2 = device_setup(eng, 5, S)
    want = make_params(eng, 5, g5, gl5, g2, s_g2)
    small = world7["params"].downsize(5)
    same = world7["params"].downsize(7)
    try:
        assert small.k == 5 and small.handle.encode(RAW).tobytes() == want.handle.encode(RAW).tobytes()
        assert small.check() == (set(), set())
        assert same.handle.encode(RAW).tobytes() == world7["raw"]
        for k_new in (8, 0):
            with pytest.raises(_lib.PzError) as e:
                world7["params"].downsize(k_new)
            assert e.value.status == _lib.PZ_ERR_INVALID
    finally:
        for p in (want, small, same):
            p.free()


def test_bases_commit_like_srs_load_g1(eng, world7):
    rng = random.Random(23)
    col = np.array([B.fr_words(rng.randrange(B.R)) for _ in range(128)], dtype=np.uint64)
    p = world7["params"]
    for lagrange, pts in ((False, world7["g"]), (True, world7["gl"])):
        ref = eng.srs_load_g1(7, pts, lagrange)
        try:
            own = p.bases(lagrange)
            assert (own.n_points, own.window_bits, own.n_windows) == (ref.n_points, ref.window_bits, ref.n_windows)
            assert p.bases(lagrange) is own                      # built once
            got, want = eng.g1_normalize(eng.msm(own, col)), eng.g1_normalize(eng.msm(ref, col))
            assert np.array_equal(got, want) and got.any()
        finally:
            ref.free()
    d_g, d_gl = p.handle.points()
    assert np.array_equal(eng.download(d_g, (128, 8)), world7["g"]) and np.array_equal(eng.download(d_gl, (128, 8)), world7["gl"])


def test_info_feeds_vk_create(eng, world7):
    p = world7["params"]
    g0, g2, s_g2 = p.handle.info()
    assert np.array_equal(g0, world7["g"][0]) and g2.astype("<u8").tobytes() == world7["g2"] and s_g2.astype("<u8").tobytes() == world7["s_g2"]
    assert B.g2_from_words(g2) == B.G2 and B.g2_from_words(s_g2) == B.g2_mul(B.G2, S)
    vp = p.verifier_params()
    assert np.array_equal(vp.g0, g0) and np.array_equal(vp.g2, g2) and np.array_equal(vp.s_g2, s_g2)
    pts = world7["g"][:6]                                        # any curve points will do for the key's commitments
    vk = eng.vk_create(7, 5, 1, 1, pts[:3], pts[3:6], g0, g2, s_g2)
    assert vk.commitment_words > 0
    vk.free()


# ---------------------------------------------------------------------------------------------------------------- the compiled driver
def test_params_tool_checks_converts_and_downsizes(eng, world7, tmp_path):
    exe = build_params_tool(tmp_path)
    raw = world7["raw"]
    honest, tampered = tmp_path / "honest.srs", tmp_path / "tampered.srs"
    honest.write_bytes(raw)
    t = bytearray(raw)
    t[4 + 64 * 5: 4 + 64 * 6] = raw[4 + 64 * 6: 4 + 64 * 7]      # g[5] <- g[6]
    tampered.write_bytes(bytes(t))
    run = lambda *a: subprocess.run([exe, *[str(x) for x in a]], capture_output=True, text=True)
    r = run("check", honest)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == {"k": 7, "format": "raw", "failed": [], "skipped": []}
    r = run("check", tampered)
    assert r.returncode == 1 and "BAD_POWERS" in json.loads(r.stdout)["failed"], (r.stdout, r.stderr)
    proc, back, small = tmp_path / "p.srs", tmp_path / "back.srs", tmp_path / "k5.srs"
    assert run("convert", honest, "processed", proc).returncode == 0
    assert proc.read_bytes() == world7["params"].handle.encode(PROCESSED).tobytes()
    assert run("convert", proc, "raw", back).returncode == 0 and back.read_bytes() == raw
    assert run("downsize", proc, 5, small).returncode == 0
    q = eng.params_decode(small.read_bytes(), PROCESSED)
    try:
        assert q.k == 5 and q.check() == (0, 0)
    finally:
        q.free()
    assert run("downsize", honest, 8, small).returncode == 2
