"""Test-side helper of tests/test_gpu_tally.py's regression guard: SHA-256 digests of the add circuit's (kind 1) structure arrays, from
both generators, and of one seeded stepper proof's wire bytes, at 128-bit n / 64-bit limbs / lookup_bits 11 / k = 12.  Uses only what
the library had before the tally; the committed digests (tests/golden/tally_kind1_regression.json) were taken from that library."""
import hashlib

import numpy as np

from oracle import pyref as P

BITS, W, LB, K = 128, 64, 11, 12


def _sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digests(eng, cref) -> dict:
    import torch
    from paillier_halo2_amd import circuit_structure as CS
    from paillier_halo2_amd import prover, prover_native
    from paillier_halo2_amd import verifier as PV

    n = 1 << K
    Ln, L = BITS // W, 2 * (BITS // W)
    nn = P.synth_paillier_inputs(BITS, 0x7a40)[0]
    c1, c2 = (nn * 3 + 17) % (1 << BITS), (nn * 5 + 29) % (1 << BITS)
    res = P.paillier_add_native(nn, c1, c2)
    out = {}
    sa = CS.stream_structure("add", BITS, W, LB)
    cs, starts = CS.columns(sa, K, LB, device="cpu")
    out["python_structure"] = _sha(cs.selectors, cs.map_col, cs.map_row, starts, np.asarray([int(c) % (1 << 64) for c in cs.constants], dtype=np.uint64))
    ns = prover_native.NativeStructure(eng, "add", BITS, W, LB, K)
    F = lambda v: cref.fr_ints_to_mont([v % P.FR_R])[0]
    d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    eng.srs_setup_g1_dev(K, F(0x1234567 ** 5), F(P.fr_omega(K)), d_g.data_ptr(), d_gl.data_ptr())
    eng.sync()
    bl, bm = eng.load_bases_dev(d_gl.data_ptr(), n), eng.load_bases_dev(d_g.data_ptr(), n)
    key = None
    try:
        sel, mc, mr = ns.download()
        out["native_structure"] = _sha(sel, mc, mr, ns.starts(), np.asarray([c % (1 << 64) for c in ns.constants()], dtype=np.uint64))
        lim = cref.int_to_limbs
        q, rem = eng.mul_mod(L, lim(c1, L), lim(c2, L), lim(nn * nn, L))
        d_steps = torch.from_numpy(np.stack([lim(c1, L), lim(c2, L), q, rem]).astype(np.int64)).cuda().view(1, 4, L)
        d_mod = torch.from_numpy(lim(nn * nn, L).astype(np.int64)).cuda()
        cols = torch.zeros((ns.m, n, 4), dtype=torch.int64, device="cuda")
        inputs = np.concatenate([lim(nn, Ln), lim(0, Ln), lim(c1, Ln), lim(c2, Ln), lim(res, L)])
        eng.circuit_expand_cols_dev(1, Ln, W, LB, inputs, d_steps.data_ptr(), 0, 0, d_mod.data_ptr(), cols.data_ptr(), cols[ns.n_adv].data_ptr(),
                                    ns.d_starts, ns.n_adv, ns.max_rows, ns.max_rows, n)
        eng.sync()
        out["witness"] = _sha(cols.cpu().numpy())
        key = ns.key(bl, bm, tile=8)
        pr = prover_native.create_proof(key, cols.data_ptr(), prover.HashTranscript(b"kind1-regression"), seed=3)
        assert pr.h_degree_ok
        vk_c = key.vk_commitments()
        vk = PV.VerifyingKey(K, 6, ns.n_adv, ns.n_lk, -(-ns.m // 2), vk_c["fixed"], vk_c["sigma"])
        out["proof"] = hashlib.sha256(PV.proof_to_bytes(eng, vk, pr)).hexdigest()
    finally:
        if key is not None:
            key.free()
        ns.free()
        bl.free()
        bm.free()
    return out
