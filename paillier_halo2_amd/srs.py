"""ParamsKZG file format (the `./params/kzg_bn254_{k}.srs` files halo2-lib's `gen_srs` caches; the reference
git-ignores that directory, `/root/reference/.gitignore:4`, and reaches `gen_srs` through `bench.rs:161-171`).

Layout restated from halo2-axiom `ParamsKZG::write` == `write_custom(.., SerdeFormat::RawBytes)` (dependency
behaviour, SURVEY tag [D]; the reference ships no sample file, so the format is unpinned here):

    u32 LE   k
    2^k x 64 B   g[i]           G1Affine, RawBytes: x then y, each the 4 x u64 LE Montgomery limbs
    2^k x 64 B   g_lagrange[i]  same
    128 B        g2             G2Affine RawBytes (x.c0, x.c1, y.c0, y.c1)
    128 B        s_g2

RawBytes is exactly the C ABI's in-memory point layout (include/pz.h), so the point sections are handed to
`pz_bases_load_g1` without conversion; `read` memory-maps them (a k = 26 file is 8.6 GB).  The reader checks
sizes; on-curve validation of what it returns is `Engine.g1_check` (on the device), the analogue of the
`is_on_curve` assertion inside halo2curves' `read_raw`.  The G2 pair (g2, s_g2) is what a KZG verifier needs: `setup_g2`
makes it for a toxic scalar as `ParamsKZG::setup` does; `paillier_halo2_amd.verifier` checks proofs against it.
"""
from __future__ import annotations

import os
import struct
from dataclasses import dataclass

import numpy as np

G2_BYTES = 128


@dataclass
class ParamsKZG:
    k: int
    g: np.ndarray            # (2^k, 8) uint64
    g_lagrange: np.ndarray   # (2^k, 8) uint64
    g2: bytes
    s_g2: bytes

    @property
    def n(self) -> int:
        return 1 << self.k


def file_size(k: int) -> int:
    return 4 + 2 * (64 << k) + 2 * G2_BYTES


def setup_g2(eng, s) -> tuple:
    """(g2, s_g2) of `ParamsKZG::setup` for the toxic scalar s (Fr Montgomery, 4 words: what `pz_srs_setup_g1_dev` takes), as the
    128-byte RawBytes values `write_params_kzg` accepts: g2 = halo2curves' G2 generator (`pz_g2_generator`), s_g2 = [s] g2 computed
    on the device (`pz_g2_mul_dev`)."""
    g2 = eng.g2_generator()
    d = eng.dev_alloc(2 * G2_BYTES + 32)
    try:
        eng.upload(d, g2)
        eng.upload(d + G2_BYTES, np.ascontiguousarray(s, dtype=np.uint64).reshape(4))
        eng.g2_mul_dev(d, d + G2_BYTES, 1, d + G2_BYTES + 32)
        s_g2 = eng.download(d + G2_BYTES + 32, 16)
    finally:
        eng.dev_free(d)
    return g2.astype("<u8").tobytes(), s_g2.astype("<u8").tobytes()


def write_params_kzg(path: str, k: int, g, g_lagrange, g2: bytes = bytes(G2_BYTES), s_g2: bytes = bytes(G2_BYTES)) -> None:
    n = 1 << k
    g = np.ascontiguousarray(g, dtype=np.uint64).reshape(-1, 8)
    gl = np.ascontiguousarray(g_lagrange, dtype=np.uint64).reshape(-1, 8)
    if g.shape[0] != n or gl.shape[0] != n:
        raise ValueError("g and g_lagrange must hold 2^k points")
    if len(g2) != G2_BYTES or len(s_g2) != G2_BYTES:
        raise ValueError("g2 / s_g2 are 128 raw bytes each")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", k))
        f.write(g.astype("<u8", copy=False).tobytes())
        f.write(gl.astype("<u8", copy=False).tobytes())
        f.write(g2)
        f.write(s_g2)


def read_params_kzg(path: str, expect_k: int | None = None) -> ParamsKZG:
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(4)
        if len(head) != 4:
            raise ValueError("truncated ParamsKZG file (no header)")
        (k,) = struct.unpack("<I", head)
        if k > 28:
            raise ValueError("implausible k = %d in ParamsKZG header" % k)
        if expect_k is not None and k != expect_k:
            raise ValueError("ParamsKZG file is for k = %d, expected %d" % (k, expect_k))
        if size != file_size(k):
            raise ValueError("ParamsKZG file for k = %d must be %d bytes, found %d (not the RawBytes format?)" % (k, file_size(k), size))
        n = 1 << k
        f.seek(4 + 2 * 64 * n)
        g2 = f.read(G2_BYTES)
        s_g2 = f.read(G2_BYTES)
    g = np.memmap(path, dtype="<u8", mode="r", offset=4, shape=(n, 8))
    gl = np.memmap(path, dtype="<u8", mode="r", offset=4 + 64 * n, shape=(n, 8))
    return ParamsKZG(k, g, gl, g2, s_g2)


# ---- the params file through the library (include/pz.h: pz_params_*) ------------------------------------------
# Everything above reads and writes RawBytes in Python and trusts what it reads.  The functions below hand the file's bytes to the C ABI:
# every point is decoded and checked on the device, SerdeFormat::Processed files are read and written too, and Params.check() says whether
# g, g_lagrange, g2 and s_g2 belong to one structured reference string.
FORMAT_NAMES = {"processed": 0, "raw": 1, "raw_unchecked": 2}   # halo2's SerdeFormat; the values are include/pz.h's PZ_SERDE_*


def _format(fmt) -> int:
    if isinstance(fmt, str):
        if fmt.lower() not in FORMAT_NAMES:
            raise ValueError("format: processed | raw | raw_unchecked")
        return FORMAT_NAMES[fmt.lower()]
    if fmt not in FORMAT_NAMES.values():
        raise ValueError("format: 0 (processed), 1 (raw) or 2 (raw_unchecked)")
    return int(fmt)


class Params:
    """A ParamsKZG held by the library on the device (engine.ParamsHandle) with halo2's operations on it."""

    def __init__(self, handle):
        self.handle = handle

    @property
    def k(self) -> int:
        return self.handle.k

    @classmethod
    def from_dev(cls, eng, k: int, d_g: int, d_g_lagrange: int, g2, s_g2) -> "Params":
        """from pz_srs_setup_g1_dev's device points and setup_g2's pair (d_g_lagrange = 0: derived from g on the device)"""
        return cls(eng.params_from_dev(k, d_g, d_g_lagrange, g2, s_g2))

    def check(self):
        """-> (failed, skipped): sets of the names BAD_G1, BAD_G2, BAD_G0, BAD_POWERS, BAD_LAGRANGE.  An empty `failed` means the four
        sections form one well-formed SRS for some s -- not that nobody knows s."""
        from ._lib import PARAMS_CHECK_NAMES

        f, s = self.handle.check()
        names = lambda bits: {n for b, n in PARAMS_CHECK_NAMES.items() if bits & b}
        return names(f), names(s)

    def downsize(self, k: int) -> "Params":
        """ParamsKZG::downsize: the first 2^k powers, g_lagrange recomputed for the smaller domain, the G2 pair kept"""
        return Params(self.handle.downsize(k))

    def write(self, path: str, fmt="raw") -> None:
        """ParamsKZG::write_custom"""
        data = self.handle.encode(_format(fmt))
        with open(path, "wb") as f:
            f.write(data.tobytes())

    def bases(self, lagrange: bool):
        """the window table of g (False) or g_lagrange (True) for the MSM entry points; owned by this object"""
        return self.handle.bases(lagrange)

    def verifier_params(self):
        from .verifier import VerifierParams

        return VerifierParams.from_parts(*self.handle.info())

    def free(self):
        self.handle.free()


def load_params(eng, path: str, fmt=None) -> Params:
    """ParamsKZG::read_custom through the C ABI: the file is memory-mapped and decoded on the device chunk by chunk; in the formats
    "processed" and "raw" every point is checked and a bad one raises PzError (its n_bad = how many).  fmt = None takes the format from
    the file's size, which is unambiguous for the k in its header ("raw" for a RawBytes file: pass "raw_unchecked" to skip the checks)."""
    size = os.path.getsize(path)
    if size < 4:
        raise ValueError("truncated ParamsKZG file (no header)")
    with open(path, "rb") as f:
        (k,) = struct.unpack("<I", f.read(4))
    if fmt is None:
        if not 1 <= k <= 28:
            raise ValueError("implausible k = %d in ParamsKZG header" % k)
        sizes = {eng.params_file_bytes(k, v): v for v in (FORMAT_NAMES["processed"], FORMAT_NAMES["raw"])}
        if size not in sizes:
            raise ValueError("ParamsKZG file for k = %d must be %s bytes, found %d" % (k, " or ".join(str(b) for b in sorted(sizes)), size))
        fmt = sizes[size]
    data = np.memmap(path, dtype=np.uint8, mode="r")
    return Params(eng.params_decode(data, _format(fmt)))
