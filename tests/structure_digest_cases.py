"""Test-side helper shared by tests/test_structure_digests.py, tests/test_gpu_structure_kinds.py and the recorder
tests/golden/make_structure_digests.py: ONE list of small shapes that reaches every branch of the two structure generators (a single
entry -- no sum, no tree, no network --, an odd tree level, more than one limb of s, slots = 1 and slots > 1), and the SHA-256 digests
of what the generators give on them.  The committed digests (tests/golden/structure_digests.json) were taken from the library BEFORE
the generators were split into shared parts: the split must not move a cell."""
import hashlib

import numpy as np

from oracle import pyref as P

BITS, W, LB = 128, 64, 10
K_MIN, MAX_ADVICE = 12, 256
EXP_G = 0x5a5


def _n() -> int:
    return P.synth_paillier_inputs(BITS, 0x11)[0]


def cases():
    """-> [(id, kind, the generator's keyword arguments)]"""
    n = _n()
    out = [("encrypt", "encrypt", dict(exp_g=EXP_G, exp_r=n)), ("add", "add", {}), ("encrypt_uniform", "encrypt_uniform", dict(exp_r=n)),
           ("decrypt", "decrypt", dict(exp_r=n))]
    out += [("tally-%d" % c, "tally", dict(count=c)) for c in (2, 5)]
    out += [("wtally-%d-%d" % s, "wtally", dict(count=s[0], w_bits=s[1])) for s in ((1, 1), (3, 2), (5, 3))]
    out += [("ballot-%d-%d" % s, "ballot", dict(count=s[0], m_bits=s[1], exp_r=n)) for s in ((1, 1), (3, 2))]
    out += [("partial-1", "partial", dict(count=1))]
    out += [("mix-%d" % c, "mix", dict(count=c, exp_r=n)) for c in (1, 2, 4)]
    out += [("sballot-%d-%d-%d" % s, "sballot", dict(count=s[0], m_bits=s[1], s_limbs=s[2])) for s in ((1, 1, 3), (2, 2, 1))]
    out += [("smix-%d-%d" % s, "smix", dict(count=s[0], s_limbs=s[1])) for s in ((1, 2), (2, 4), (4, 1))]
    out += [("pballot-%d-%d-%d-%d" % s, "pballot", dict(count=s[0], slots=s[1], m_bits=s[2], s_limbs=s[3])) for s in ((1, 1, 1, 2), (2, 3, 2, 1))]
    return out


CASES = cases()
IDS = [c[0] for c in CASES]


def _words256(values) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def _ints(*values) -> bytes:
    return np.asarray([int(v) for v in values], dtype=np.int64).tobytes()


def _host(a, dtype) -> bytes:
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()            # (a tensor of the device= path)
    return np.ascontiguousarray(a, dtype=dtype).tobytes()


def stream(kind, kw, device=None):
    from paillier_halo2_amd import circuit_structure as CS

    return CS.stream_structure(kind, BITS, W, LB, device=device, **kw)


def stream_digest(sa) -> str:
    """SHA-256 over everything stream_structure returns"""
    h = hashlib.sha256()
    h.update(_host(sa.src, np.int64))
    h.update(_host(sa.gate_mask, np.uint8))
    h.update(_host(sa.lookup_src, np.int64))
    h.update(_words256(sa.constants))
    h.update(_ints(sa.n_cells, sa.result_cell, sa.n_steps_g, sa.n_steps_r))
    h.update(_host(sa.public_cells, np.int64))
    return h.hexdigest()


def pick_k(sa) -> int:
    """the smallest k >= 12 at which the stream needs at most 256 advice columns"""
    from paillier_halo2_amd import layout

    k = K_MIN
    while True:
        rb = layout.row_budget(k)
        filled = layout.break_points(sa.gate_mask, rb.max_rows).shape[0] - 1
        if rb.columns_for(sa.n_cells, filled=filled) <= MAX_ADVICE:
            return k
        k += 1


def native(eng, kind, kw, k, expose):
    from paillier_halo2_amd import prover_native

    return prover_native.NativeStructure(eng, kind, BITS, W, LB, k, expose=expose, **kw)


def native_digest(ns) -> str:
    """SHA-256 over everything the native generator gives: counts, constants, starts, selectors, the permutation, the exposed cells"""
    h = hashlib.sha256()
    h.update(_ints(ns.n_cells, ns.n_lookups, ns.n_steps_g, ns.n_steps_r, ns.n_adv, ns.n_adv_used, ns.n_lk, ns.max_rows, ns.n_instance,
                   ns.n_public))
    h.update(_words256(ns.constants()))
    h.update(np.ascontiguousarray(ns.starts(), dtype=np.uint64).tobytes())
    for a in ns.download():
        h.update(np.ascontiguousarray(a).tobytes())
    if ns.n_public:
        h.update(_ints(*[v for cell in ns.public_cells() for v in cell]))
    return h.hexdigest()
