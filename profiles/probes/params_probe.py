"""ParamsKZG files through the C ABI (csrc/pz_params.hip, pz_params.cpp) at k = 17.
  python profiles/probes/params_probe.py [k] [out.json]
An SRS is set up on the device (pz_srs_setup_g1_dev, srs.setup_g2), encoded to RAW and PROCESSED file bytes in host memory, and then, warmed,
as ranges over five repeats of the whole call (wall time, the call synchronises):
  decode_raw_ms / decode_processed_ms   pz_params_decode of those bytes (upload, per-point check or decompression, the G2 pair)
  load_g1_ms                            the baseline: pz_srs_load_g1 of the same 2^k points of g (upload + window table, no check)
  check_ms                              pz_params_check of an honest object, its window tables already built; check_first_ms: the call that
                                        builds them
  tables_bytes                          device memory the object holds above its 2 x 2^k points once both tables exist (pz_dev_mem_info
                                        before and after the first check, its workspaces freed again) -- beside the size of the two tables as
                                        pz_bases_info gives it
Prints one JSON line; with a second argument also writes it there."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import paillier_halo2_amd as pz
from paillier_halo2_amd import _lib, consts, srs

REPEATS = 5


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def ms_range(fn, cleanup=lambda r: None):
    ms = []
    for _ in range(REPEATS):
        t, r = timed(fn)
        cleanup(r)
        ms.append(t)
    return [round(min(ms), 1), round(max(ms), 1)]


def main(k, out_path):
    eng = pz.Engine(0)
    n = 1 << k
    M = consts.fr_mont_limbs
    s_tox = 0x5EED5EED5EED5EED5EED5EED5EED5EED
    d = eng.dev_alloc(2 * n * 64)
    eng.srs_setup_g1_dev(k, M(s_tox), M(consts.fr_omega(k)), d, d + n * 64)
    g2, s_g2 = srs.setup_g2(eng, M(s_tox))
    p = eng.params_from_dev(k, d, d + n * 64, g2, s_g2)
    g_host = eng.download(d, (n, 8))
    eng.dev_free(d)
    raw, proc = p.encode(_lib.PZ_SERDE_RAW), p.encode(_lib.PZ_SERDE_PROCESSED)
    p.free()
    out = {"k": k, "raw_bytes": int(raw.size), "processed_bytes": int(proc.size), "repeats": REPEATS}
    free = lambda h: h.free()
    eng.params_decode(raw, _lib.PZ_SERDE_RAW).free()                 # warm-up: the library's workspaces, the pinned staging
    eng.params_decode(proc, _lib.PZ_SERDE_PROCESSED).free()
    eng.srs_load_g1(k, g_host).free()
    out["decode_raw_ms"] = ms_range(lambda: eng.params_decode(raw, _lib.PZ_SERDE_RAW), free)
    out["decode_raw_unchecked_ms"] = ms_range(lambda: eng.params_decode(raw, _lib.PZ_SERDE_RAW_UNCHECKED), free)
    out["decode_processed_ms"] = ms_range(lambda: eng.params_decode(proc, _lib.PZ_SERDE_PROCESSED), free)
    out["load_g1_ms"] = ms_range(lambda: eng.srs_load_g1(k, g_host), free)
    w = eng.params_decode(raw, _lib.PZ_SERDE_RAW)                    # grows the context's MSM / NTT workspaces to this size once,
    assert w.check() == (0, 0)                                       # so that the memory difference below is the tables alone
    w.free()
    q = eng.params_decode(raw, _lib.PZ_SERDE_RAW)
    eng.sync()
    free0, _ = eng.dev_mem_info()
    t, verdict = timed(q.check)
    assert verdict == (0, 0), verdict
    out["check_first_ms"] = round(t, 1)
    free1, _ = eng.dev_mem_info()
    bg, bl = q.bases(False), q.bases(True)
    out["tables_bytes"] = int(free0 - free1)
    out["tables_bytes_from_info"] = 64 * (bg.n_windows * bg.n_points + bl.n_windows * bl.n_points)
    out["window_bits"] = bg.window_bits
    out["points_bytes"] = 2 * n * 64
    out["check_ms"] = ms_range(q.check)
    # the same object with one point moved: the verdict the check exists for, at this size
    t = bytearray(raw.tobytes())
    t[4 + 64 * 5: 4 + 64 * 6] = t[4 + 64 * 6: 4 + 64 * 7]
    bad = eng.params_decode(bytes(t), _lib.PZ_SERDE_RAW)
    out["tampered_verdict"] = sorted(_lib.PARAMS_CHECK_NAMES[b] for b in _lib.PARAMS_CHECK_NAMES if bad.check()[0] & b)
    bad.free()
    q.free()
    eng.close()
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 17, sys.argv[2] if len(sys.argv) > 2 else None)
