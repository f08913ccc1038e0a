"""Test helper (not product code): a ParamsKZG in Python integers, built independently of paillier_halo2_amd from a scalar s, and the three
file formats of DESIGN.md section 15.4 (halo2's write_custom: u32 k | g[2^k] | g_lagrange[2^k] | g2 | s_g2).

    g[i]          = [s^i] G
    g_lagrange[i] = [L_i(s)] G,  L_i(s) = (s^n - 1) omega^i / (n (s - omega^i))   (the closed form of include/pz.h)
    g2            = halo2curves' G2 generator,  s_g2 = [s] g2

G1 points go through tests/wire_ref.py, G2 points through tests/g2_wire_ref.py and tests/bn254_pairing_ref.py.  Small k only (Python)."""
import struct
from dataclasses import dataclass
from typing import List

from tests import bn254_pairing_ref as B
from tests import g2_wire_ref as G2W
from tests import wire_ref as W

R = W.R
ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C   # halo2curves Fr::ROOT_OF_UNITY, order 2^28
assert pow(ROOT_OF_UNITY, 1 << 28, R) == 1 and pow(ROOT_OF_UNITY, 1 << 27, R) != 1
PROCESSED, RAW, RAW_UNCHECKED = 0, 1, 2


def omega(k: int) -> int:
    return pow(ROOT_OF_UNITY, 1 << (28 - k), R)


@dataclass
class Srs:
    k: int
    g: List            # 2^k G1 points, (x, y) or None
    g_lagrange: List
    g2: tuple          # ((x0, x1), (y0, y1)) or None
    s_g2: tuple


def setup(k: int, s: int, s2=None) -> Srs:
    """s2: the scalar of the G2 side, if it is to differ from the G1 side's (a file assembled from two setups)"""
    n, w = 1 << k, omega(k)
    g = [W.mul(pow(s, i, R)) for i in range(n)]
    zn = (pow(s, n, R) - 1) % R
    gl = [W.mul(zn * pow(w, i, R) * pow(n * (s - pow(w, i, R)), -1, R) % R) for i in range(n)]
    return Srs(k, g, gl, B.G2, B.g2_mul(B.G2, s if s2 is None else s2))


def file_bytes(k: int, fmt: int) -> int:
    return 4 + 2 * ((32 if fmt == PROCESSED else 64) << k) + 2 * (64 if fmt == PROCESSED else 128)


def _words_bytes(words) -> bytes:
    return b"".join(struct.pack("<Q", int(w)) for w in words)


def encode(srs: Srs, fmt: int) -> bytes:
    out = struct.pack("<I", srs.k)
    if fmt == PROCESSED:
        out += b"".join(W.compress(p) for p in srs.g + srs.g_lagrange)
        out += G2W.compress(srs.g2) + G2W.compress(srs.s_g2)
    else:
        out += b"".join(_words_bytes(W.point_words(p)) for p in srs.g + srs.g_lagrange)
        out += _words_bytes(B.g2_words(srs.g2)) + _words_bytes(B.g2_words(srs.s_g2))
    assert len(out) == file_bytes(srs.k, fmt)
    return out


def decode(data: bytes, fmt: int) -> Srs:
    """every point must decode (processed) and lie on its curve, as halo2's read_custom asserts but for RawBytesUnchecked"""
    (k,) = struct.unpack("<I", data[:4])
    assert len(data) == file_bytes(k, fmt)
    n = 1 << k
    pb, qb = (32, 64) if fmt == PROCESSED else (64, 128)
    off = 4
    pts = []
    for i in range(2 * n):
        chunk = data[off + pb * i: off + pb * (i + 1)]
        if fmt == PROCESSED:
            st, p = W.decompress(chunk)
            assert st == W.OK
        else:
            (p,) = W.points_from_words(struct.unpack("<8Q", chunk))
            assert fmt == RAW_UNCHECKED or p is None or (p[1] * p[1] - p[0] ** 3 - 3) % W.P == 0
        pts.append(p)
    off += 2 * pb * n
    qs = []
    for i in range(2):
        chunk = data[off + qb * i: off + qb * (i + 1)]
        if fmt == PROCESSED:
            st, q = G2W.decompress(chunk)
            assert st == G2W.OK
        else:
            q = B.g2_from_words(struct.unpack("<16Q", chunk))
            assert fmt == RAW_UNCHECKED or B.g2_on_curve(q)
        qs.append(q)
    return Srs(k, pts[:n], pts[n:], qs[0], qs[1])
