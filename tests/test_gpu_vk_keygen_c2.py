"""GPU, BASELINE config c2 (2048-bit n, k = 17, lookup_bits 16, minimum_rows 20; the structure from the library's generator): keygen_vk's
key equals the commitments of a proving key built from the same structure, and it is derived in bounded memory -- under pz_dev_arena, with
the MSM workspaces warm, the call's transient device memory stays below the size of the sigma columns alone (m 2^k 32 bytes = 13.1 GB),
which the proving-key path cannot avoid holding."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BITS, K, LB, SEED, TILE = 2048, 17, 16, 0x5043, 64
GIB = 1 << 30


def test_c2_key_equals_the_proving_keys_in_bounded_memory():
    import torch

    import bench
    import paillier_halo2_amd as pz
    from paillier_halo2_amd import consts, prover_native
    from paillier_halo2_amd import verifier as PV

    eng = pz.Engine(0)
    eng.bind_torch_stream()
    ns = key = bl = bm = None
    try:
        n = 1 << K
        s_tox = random.Random(SEED ^ 0x535253).randrange(2, consts.FR_R)
        M = consts.fr_mont_limbs
        d_g = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        d_gl = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        eng.srs_setup_g1_dev(K, M(s_tox), M(consts.fr_omega(K)), d_g.data_ptr(), d_gl.data_ptr())
        eng.sync()
        bl, bm = eng.load_bases_dev(d_gl.data_ptr(), n), eng.load_bases_dev(d_g.data_ptr(), n)
        del d_g, d_gl
        nn, g, m, r = bench.synth_inputs(BITS, SEED)
        ns = prover_native.NativeStructure(eng, "encrypt", BITS, 64, LB, K, exp_g=m, exp_r=nn, minimum_rows=20)
        assert (ns.n_adv, ns.n_lk) == (3034, 84)
        # the arena AFTER the bases and the structure (their temporaries would otherwise have raised its peak before the measured call)
        free, _ = eng.dev_mem_info()
        eng.dev_arena(min(170 * GIB, max(free - 8 * GIB, 1 * GIB)))         # what it cannot serve falls through to the driver
        # warm the MSM workspaces: TILE dense columns (scalars below 2^252, held outside the arena)
        sc = torch.randint(-(1 << 63), (1 << 63) - 1, (TILE, n, 4), dtype=torch.int64, device="cuda")
        sc[..., 3] &= 0x0FFFFFFFFFFFFFFF
        out = torch.zeros((TILE, 12), dtype=torch.int64, device="cuda")
        eng.msm_dev(bl, sc.data_ptr(), TILE, n, 4 * n, out.data_ptr())
        eng.sync()
        del sc, out
        before = eng.dev_arena_info()
        assert before["bytes"] > 0, before
        vk = PV.VerifyingKey.from_structure(eng, ns, bl, tile=TILE)
        after = eng.dev_arena_info()
        # the peak is a high-water mark since the arena was made: measured from the live bytes at the call's start it bounds the call's
        # transient from above whatever the warm-up left behind (it equals the rise of the peak when the warm-up freed nothing)
        rise = after["peak"] - before["used"]
        sigma_bytes = ns.m * n * 32
        print("\nkeygen_vk at c2: arena peak above the live bytes at the start %.1f MB (rise of the peak itself %.1f MB, live bytes %+.1f MB); "
              "the sigma columns alone: %.1f MB" % (rise / 1e6, (after["peak"] - before["peak"]) / 1e6, (after["used"] - before["used"]) / 1e6,
                                                    sigma_bytes / 1e6))
        assert after["missed"] == before["missed"], "an allocation of the call went past the arena: the peak does not account for it"
        assert rise < sigma_bytes, (rise, sigma_bytes)
        # the same commitments as a proving key made from the same structure
        key = ns.key(bl, bm)
        c = key.vk_commitments()
        assert (vk.k, vk.n_adv, vk.n_lk, vk.n_sets) == (K, ns.n_adv, ns.n_lk, key.n_sets)
        assert np.array_equal(vk.fixed, c["fixed"]) and np.array_equal(vk.sigma, c["sigma"])
    finally:
        if key is not None:
            key.free()
        if ns is not None:
            ns.free()
        for b in (bl, bm):
            if b is not None:
                b.free()
        eng.close()
