"""keygen_vk at BASELINE config c2 (2048-bit n, k = 17, lookup_bits 16, minimum_rows 20).  One warmed process, every
pair alternated, REPEATS repeats, ranges reported.
  python profiles/probes/vk_keygen_probe.py [out.json]
        (b) the 3034 selector columns through pz_g1_commit_mask_dev -- at every chunk size (PZ_MASK_CHUNK) -- against pz_fr_from_mask_dev +
            pz_msm_g1_dev on the same masks through a tile buffer (64 and 512 columns), results compared after normalisation; set rows
            counted from the masks -> additions per second;
        (a) pz_vk_keygen_dev against pz_pk_create_dev on the same structure: wall time of each and, under pz_dev_arena, how far each
            raises the arena's peak above the live bytes at its start.
  python profiles/probes/vk_keygen_probe.py --kernel
        the mask kernel alone, a few launches at the default chunk: run it under
        `rocprofv3 --kernel-trace --stats -- python profiles/probes/vk_keygen_probe.py --kernel` for k_commit_mask's own time."""
import json, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import paillier_halo2_amd as pz

BITS, K, LB, SEED = 2048, 17, 16, 0x5043
REPEATS = 5
GIB = 1 << 30
rng_ = lambda v: [round(min(v), 2), round(max(v), 2)]


def setup(eng, torch):
    import bench
    from paillier_halo2_amd import consts, prover_native

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
    return bl, bm, ns


def mask_call(eng, bl, ns, d_out):
    eng.g1_commit_mask_dev(bl, ns.d_selectors, ns.n_adv, 1 << K, 1 << K, d_out)
    eng.sync()


def msm_path(eng, bl, ns, buf, tile, d_out):
    n, A = 1 << K, ns.n_adv
    for c0 in range(0, A, tile):
        nc = min(tile, A - c0)
        eng.fr_from_mask_dev(ns.d_selectors + c0 * n, nc * n, buf.data_ptr())
        eng.msm_dev(bl, buf.data_ptr(), nc, n, 4 * n, d_out + c0 * 96)
    eng.sync()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main(out_path):
    import torch
    from paillier_halo2_amd import verifier as PV

    eng = pz.Engine(0)
    eng.bind_torch_stream()
    bl, bm, ns = setup(eng, torch)
    n, A, m = 1 << K, ns.n_adv, ns.m
    sel = torch.zeros((A, n), dtype=torch.uint8, device="cuda")
    eng.dev_copy(sel.data_ptr(), ns.d_selectors, A * n)
    eng.sync()
    set_rows = int(sel.count_nonzero().item())
    del sel
    out = {"config": "c2", "k": K, "n_adv": A, "n_lk": ns.n_lk, "m": m, "repeats": REPEATS, "selector_set_rows": set_rows,
           "selector_density": round(set_rows / (A * n), 4)}
    # ---- (b) selectors: the mask kernel against from_mask + the general MSM
    o_mask = torch.zeros((A, 12), dtype=torch.int64, device="cuda")
    o_msm = torch.zeros((A, 12), dtype=torch.int64, device="cuda")
    bufs = {t: torch.zeros((t, n, 4), dtype=torch.int64, device="cuda") for t in (64, 512)}
    chunks = (4096, 8192, 16384, 32768)
    for t in bufs:
        msm_path(eng, bl, ns, bufs[t], t, o_msm.data_ptr())           # warm-up: workspaces
    for c in chunks:
        os.environ["PZ_MASK_CHUNK"] = str(c)
        mask_call(eng, bl, ns, o_mask.data_ptr())
    same = np.array_equal(eng.g1_normalize(o_mask.cpu().numpy().view(np.uint64)), eng.g1_normalize(o_msm.cpu().numpy().view(np.uint64)))
    t_mask = {c: [] for c in chunks}
    t_msm = {t: [] for t in bufs}
    for _ in range(REPEATS):
        for c in chunks:
            os.environ["PZ_MASK_CHUNK"] = str(c)
            t_mask[c].append(timed(lambda: mask_call(eng, bl, ns, o_mask.data_ptr())))
        for t in bufs:
            t_msm[t].append(timed(lambda: msm_path(eng, bl, ns, bufs[t], t, o_msm.data_ptr())))
    del os.environ["PZ_MASK_CHUNK"]
    out["selectors"] = {"same_commitments": bool(same),
                        "commit_mask_ms_by_chunk": {str(c): rng_(t_mask[c]) for c in chunks},
                        "from_mask_plus_msm_ms_by_tile": {str(t): rng_(t_msm[t]) for t in bufs},
                        "commit_mask_additions_per_s_by_chunk": {str(c): round(set_rows / (min(t_mask[c]) * 1e-3), 0) for c in chunks}}
    print(json.dumps(out["selectors"]), flush=True)
    del bufs, o_mask, o_msm
    torch.cuda.empty_cache()
    # ---- (a) keygen_vk against the proving key's keygen, same structure, under an arena
    vk = PV.VerifyingKey.from_structure(eng, ns, bl)                   # warm-up BEFORE the arena: the library's workspaces stay outside it
    free, _ = eng.dev_mem_info()
    eng.dev_arena(min(170 * GIB, max(free - 8 * GIB, 1 * GIB)))
    a0 = eng.dev_arena_info()
    vk = PV.VerifyingKey.from_structure(eng, ns, bl)                   # the first call in a fresh arena: its peak is this call's alone
    vk_peak_gb = (eng.dev_arena_info()["peak"] - a0["used"]) / 1e9
    ns.key(bl, bm).free()                                              # warm-up of the proving key's keygen (the arena's first touch)
    t_vk, t_pk, peak_pk, equal = [], [], [], True
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        vk = PV.VerifyingKey.from_structure(eng, ns, bl)
        t_vk.append((time.perf_counter() - t0) * 1e3)
        a1 = eng.dev_arena_info()
        t0 = time.perf_counter()
        key = ns.key(bl, bm)
        t_pk.append((time.perf_counter() - t0) * 1e3)
        a2 = eng.dev_arena_info()
        c = key.vk_commitments()
        equal = equal and np.array_equal(vk.fixed, c["fixed"]) and np.array_equal(vk.sigma, c["sigma"])
        key.free()
        peak_pk.append((a2["peak"] - a1["used"]) / 1e9)               # (the arena's peak is a high-water mark: the proving key's, every time)
    out["keygen"] = {"vk_keygen_dev_ms": rng_(t_vk), "pk_create_dev_ms": rng_(t_pk), "ratio_of_minima": round(min(t_pk) / min(t_vk), 2),
                     "same_commitments": bool(equal),
                     "vk_keygen_dev_arena_peak_above_start_gb": round(vk_peak_gb, 3), "pk_create_dev_arena_peak_above_start_gb": rng_(peak_pk)}
    print(json.dumps(out["keygen"]), flush=True)
    ns.free()
    bl.free()
    bm.free()
    eng.close()
    print(json.dumps(out))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def kernel_only():
    import torch

    eng = pz.Engine(0)
    eng.bind_torch_stream()
    bl, bm, ns = setup(eng, torch)
    o = torch.zeros((ns.n_adv, 12), dtype=torch.int64, device="cuda")
    ms = [timed(lambda: mask_call(eng, bl, ns, o.data_ptr())) for _ in range(1 + REPEATS)]
    print(json.dumps({"launches": len(ms), "wall_ms_after_the_first": rng_(ms[1:])}))
    ns.free()
    bl.free()
    bm.free()
    eng.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernel":
        kernel_only()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
